"""Seeded scenes for Planar_Mapping_module's RANSAC (tests/test_plane_ransac_cpu.py, tests/test_gpu_plane_ransac.py): a planted plane patch
with Gaussian noise clipped to a quarter of dist_thresh, a share of gross outliers at least four thresholds off the plane (some of them on a
second, parallel plane), holes of erased slots (NaN positions) and -- for UPDATE -- unowned slots, and sample plans that steer the loop:
per iteration 'c' = ranks of clean points only (with an exact duplicate among them), 'd' = ranks of outliers only, 'x' = one rank out of
range, or no plan at all = the library draws."""
import numpy as np

import plane_ransac_ref as PR

DIST_THRESH = 0.02
ERROR_THRESH = 0.002


def random_plane(rng):
    nrm = rng.standard_normal(3)
    nrm /= np.linalg.norm(nrm)
    u = np.cross(nrm, [1.0, 0.0, 0.0] if abs(nrm[0]) < 0.9 else [0.0, 1.0, 0.0])
    u /= np.linalg.norm(u)
    return nrm, u, np.cross(nrm, u), rng.uniform(-4.0, 4.0, 3)


def problem(seed, n, mode=PR.CREATE, outliers=0.15, erased=0, unowned=0, plan=None, iters=8, second_plane=0.5, dist_thresh=DIST_THRESH,
            error_thresh=ERROR_THRESH, best_error_in=PR.DBL_MAX, points_per_ransac=18, nonplanar=False):
    """one plane: dict(pos_w (n, 3), flags (n,), labels (n,): 1 = generated on the planted plane and not erased, samples (iters, m) or None, ...)"""
    rng = np.random.default_rng(seed)
    nrm, u, v, origin = random_plane(rng)
    a, b = rng.uniform(-2.0, 2.0, n), rng.uniform(-2.0, 2.0, n)
    noise = np.clip(rng.normal(0.0, dist_thresh / 8.0, n), -dist_thresh / 4.0, dist_thresh / 4.0)
    is_out = rng.random(n) < outliers
    off = rng.uniform(4.0, 40.0, n) * dist_thresh * rng.choice([-1.0, 1.0], n)        # gross outliers: at least four thresholds off
    on_second = is_out & (rng.random(n) < second_plane)
    off[on_second] = 12.0 * dist_thresh                                              # a second plane's points
    h = np.where(is_out, off, noise)
    if nonplanar:
        h = rng.uniform(-1.0, 1.0, n)
        is_out[:] = True
    pos_w = origin + a[:, None] * u + b[:, None] * v + h[:, None] * nrm
    flags = np.full(n, PR.LM_OWNED, np.uint8)
    holes = rng.permutation(n)
    er, un = holes[:erased], holes[erased:erased + unowned]
    flags[er] |= PR.LM_ERASED
    pos_w[er] = np.nan                                                                # what an erased landmark holds must not matter
    flags[un] &= ~np.uint8(PR.LM_OWNED)
    if mode == PR.CREATE:
        flags[rng.random(n) < 0.5] &= ~np.uint8(PR.LM_OWNED)                          # CREATE does not read the bit
    erased_b = (flags & PR.LM_ERASED) != 0
    eligible = np.flatnonzero(~erased_b if mode == PR.CREATE else ~erased_b & ((flags & PR.LM_OWNED) != 0))
    m = PR.sample_size(mode, n, points_per_ransac)
    samples = None
    if plan is not None:
        assert len(plan) == iters
        clean = np.flatnonzero(~is_out[eligible])
        dirty = np.flatnonzero(is_out[eligible])
        samples = np.zeros((iters, m), np.int32)
        for i, kind in enumerate(plan):
            pool = clean if kind in "cx" or len(dirty) == 0 else dirty
            samples[i] = rng.choice(pool, m, replace=True)
            if m > 1:
                samples[i, 1] = samples[i, 0]                                         # an exact duplicate
            if kind == "x":
                samples[i, m // 2] = len(eligible) if i % 2 else -1
    d0 = -float(nrm @ origin)
    return dict(mode=mode, pos_w=pos_w, flags=flags, labels=(~is_out & ~erased_b).astype(np.uint8), samples=samples, iters=iters, seed=seed,
                dist_thresh=dist_thresh, error_thresh=error_thresh, best_error_in=best_error_in, equation_in=np.array([*nrm, d0]),
                points_per_ransac=points_per_ransac, m=m, margin=not nonplanar)


def run_ref(q, p=0, **kw):
    return PR.ransac(q["mode"], q["pos_w"], q["flags"], q["dist_thresh"], q["error_thresh"], points_per_ransac=q["points_per_ransac"], iters=q["iters"],
                     best_error_in=q["best_error_in"], equation_in=q["equation_in"], samples=q["samples"], seed=q["seed"], p=p, **kw)


def pack(problems, n_cap=None):
    """the problems of one call as the library's arrays (they share mode, iters, seed and whether they carry samples): dict(pos_w (P, n_cap, 3),
    flags, counts, dist_thresh, error_thresh, best_error_in, equation_in, samples (P, iters, m_cap) or None).  Slots at or above a problem's
    count hold garbage."""
    P = len(problems)
    n_cap = max(len(q["flags"]) for q in problems) if n_cap is None else n_cap
    iters = problems[0]["iters"]
    rng = np.random.default_rng(99)
    with_samples = problems[0]["samples"] is not None
    m_cap = PR.sample_size(problems[0]["mode"], n_cap, problems[0]["points_per_ransac"])
    a = dict(pos_w=rng.uniform(-9, 9, (P, n_cap, 3)), flags=rng.integers(0, 4, (P, n_cap)).astype(np.uint8), counts=np.zeros(P, np.int32),
             dist_thresh=np.zeros(P), error_thresh=np.zeros(P), best_error_in=np.zeros(P), equation_in=np.zeros((P, 4)),
             samples=np.full((P, iters, m_cap), -5, np.int32) if with_samples else None)
    for p, q in enumerate(problems):
        n = len(q["flags"])
        assert q["iters"] == iters and n <= n_cap and (q["samples"] is not None) == with_samples and q["mode"] == problems[0]["mode"]
        a["pos_w"][p, :n], a["flags"][p, :n], a["counts"][p] = q["pos_w"], q["flags"], n
        for k in ("dist_thresh", "error_thresh", "best_error_in", "equation_in"):
            a[k][p] = q[k]
        if with_samples:
            a["samples"][p, :, :q["m"]] = q["samples"]
    return a


def call_kwargs(problems, a):
    q = problems[0]
    return dict(points_per_ransac=q["points_per_ransac"], iters=q["iters"], best_error_in=a["best_error_in"], equation_in=a["equation_in"],
                samples=a["samples"], seed=q["seed"], counts=a["counts"])


# The scenes of the CPU tests, by name.  `census` names the branch each is there for (tests/test_plane_ransac_cpu.py asserts it is reached).
def scenes():
    C, U = PR.CREATE, PR.UPDATE
    S = {}
    S["gate"] = (problem(1, 10), "gate")
    S["too_few"] = (problem(2, 15), "too_few")
    S["no_eligible"] = (problem(3, 40, erased=40), "no_eligible")
    S["break_0"] = (problem(4, 120, outliers=0.1, plan="cccccccc"), "break_0")
    S["break_mid"] = (problem(5, 150, outliers=0.2, erased=7, plan="ddxcdcdc"), "break_mid")
    S["no_break"] = (problem(6, 130, outliers=0.2, plan="dcdcdcdd", error_thresh=1e-9), "above")
    S["never"] = (problem(7, 140, outliers=0.2, plan="ddddxddd"), "never")
    S["drawn"] = (problem(8, 200, outliers=0.05, erased=11, iters=50), None)
    S["drawn_heavy"] = (problem(9, 260, outliers=0.5, erased=3, iters=50), None)
    S["nonplanar"] = (problem(10, 90, nonplanar=True, iters=12), None)
    S["u_too_few"] = (problem(11, 9, mode=U), "u_invalid_few")
    S["u_no_eligible"] = (problem(12, 30, mode=U, unowned=30), "no_eligible")
    S["u_ok"] = (problem(13, 160, mode=U, outliers=0.15, erased=5, unowned=9, plan="dcdcccdc"), None)
    S["u_last_dirty"] = (problem(14, 120, mode=U, outliers=0.05, erased=4, unowned=6, plan="cccccccd"), "u_too_few_left")
    S["u_need_refinement"] = (problem(15, 100, mode=U, outliers=0.1, unowned=5, plan="cdcdcdcd", best_error_in=0.0), "u_need_refinement")
    S["u_above"] = (problem(21, 100, mode=U, outliers=0.03, plan="cdcdcdcd", error_thresh=1e-9), "u_above")
    S["u_drawn"] = (problem(17, 180, mode=U, outliers=0.02, erased=6, unowned=4, iters=20), None)
    S["best_not_last"] = (problem(18, 150, outliers=0.2, plan="cdcdddcd", error_thresh=1e-9), "best_not_last")
    S["u_best_not_last"] = (problem(19, 140, mode=U, outliers=0.1, unowned=3, plan="dccccccc", best_error_in=1.0), None)
    S["all_clean"] = (problem(20, 64, outliers=0.0, iters=5), None)
    return S


def refine_scene(seed, M, NP=5, dist_thresh=DIST_THRESH):
    """landmarks for refine_points: dict(pos_w (M, 3), lm_plane (M,), flags (M,), equation (NP, 4), active (NP,), dist_thresh).  Plane 0 is
    z = 2 exactly, so that points exactly on a plane exist; plane 1 is inactive; the normals are not all of unit length; owners include -1 and
    one row past the table; points lie on both sides, inside and outside the threshold; some are erased (NaN) or unowned."""
    rng = np.random.default_rng(seed)
    equation = np.zeros((NP, 4))
    equation[0] = [0.0, 0.0, 1.0, -2.0]
    for k in range(1, NP):
        nrm, _, _, origin = random_plane(rng)
        scale = 1.0 if k % 2 else 2.5
        equation[k] = [*(scale * nrm), -scale * float(nrm @ origin)]
    active = np.ones(NP, np.uint8)
    if NP > 1:
        active[1] = 0
    lm_plane = rng.integers(-1, NP + 1, M).astype(np.int32)
    lm_plane[0] = 0
    pos_w = np.zeros((M, 3))
    for i in range(M):
        eq = equation[min(max(lm_plane[i], 0), NP - 1)]
        nrm = eq[:3] / np.linalg.norm(eq[:3])
        x = rng.uniform(-3.0, 3.0, 3)
        x -= nrm * (float(nrm @ x) + eq[3] / np.linalg.norm(eq[:3]))                  # onto the plane
        pos_w[i] = x + nrm * rng.choice([0.3, -0.3, 1.5, -1.5, 0.0]) * dist_thresh * rng.uniform(0.5, 1.0)
    on = np.flatnonzero(lm_plane == 0)[::2]
    pos_w[on, 2] = 2.0                                                                # exactly on plane 0
    flags = np.full(M, PR.LM_OWNED, np.uint8)
    r = rng.random(M)
    flags[(r < 0.1) & (np.arange(M) > 0)] |= PR.LM_ERASED
    flags[(r > 0.9) & (np.arange(M) > 0)] &= ~np.uint8(PR.LM_OWNED)
    pos_w[(flags & PR.LM_ERASED) != 0] = np.nan
    return dict(pos_w=pos_w, lm_plane=lm_plane, flags=flags, equation=equation, active=active, dist_thresh=dist_thresh)
