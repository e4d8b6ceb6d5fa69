"""Every path launch_match can give each matcher mode (tests/test_match_plan_cpu.py pins the choice), run batched through both entries with
ragged per-problem counts and per-problem data, and compared problem by problem with the oracle on the clamped slice.  Also: crowded
windows whose truncated candidate lists run dry (the d8 shortcut and the exact rescan of both resolve kernels), overlapping query windows
(q_desc_stride), the slots beyond a problem's count (never written, on both entries), batched LBD 1-NN and odd Hamming-matrix sizes."""
import ctypes as C

import numpy as np
import pytest

import match_cases as MC
import oracle_lib as O
from plp import plp

pytestmark = pytest.mark.gpu
SF = MC.SF8
SF_LSD = MC.SF_LSD
SENT = -7                                    # what the caller left in the output slots beyond a count
G64 = plp.make_grid(640, 480)                # 64 x 48 cells: the cells path
G256 = plp.make_grid(640, 480, 256, 16)      # 256 columns: beyond k_match_prep's 255, the generic paths
STRUCT = (plp.KP_DTYPE, plp.KL_DTYPE)
FUSE = (plp.MODE_FUSE, plp.MODE_FUSE_LINE)


def ragged(rng, B, cap, shift=0):
    """0, 1, cap - 1, cap, cap + 1000 and a negative count among the first six problems, random counts in [1, cap] after them"""
    c = rng.integers(1, cap + 1, B).astype(np.int32)
    pat = [0, 1, cap - 1, cap, cap + 1000, -3]
    for b in range(min(B, 6)):
        c[b] = pat[(b + shift) % 6]
    return c


def clamp(c, cap):
    return cap if c is None else int(min(max(c, 0), cap))


class Case:
    """B problems of one mode, each generated at full capacity (the rows beyond a problem's count hold real, different data)."""

    def __init__(self, mode, probs, n_cap, m_cap, oracle, ratio=0.8, check=False, ints=None, **kw):
        self.mode, self.probs, self.n_cap, self.m_cap, self.oracle = mode, probs, n_cap, m_cap, oracle
        self.ratio, self.check, self.ints, self.kw = ratio, check, dict(ints or {}), kw
        self.B = len(probs)

    def fields(self):
        f = {k: np.ascontiguousarray(np.stack([p[k] for p in self.probs])) for k in self.probs[0]}
        f.update(self.ints)
        return f

    def plan(self):
        return plp.match_plan(self.mode, self.B, self.n_cap, self.m_cap, grid=self.kw.get("grid"), t_x_right="t_x_right" in self.probs[0],
                              t_count_hint=self.ints.get("t_count_hint", 0))

    def expect(self, b, n, m):
        p = self.probs[b]
        if n == 0 or m == 0:   # an empty side: the reference's loops do not run
            return np.full(m, -1, np.int32) if self.mode in FUSE else (np.full(n, -1, np.int32), 0)
        return self.oracle(p, n, m)


def to_device(f):
    import torch
    dev = torch.device("cuda:0")
    host = lambda k, v: np.isscalar(v) or k == "inv_level_sigma_sq"   # scalars and the host-pointer table stay
    return {k: (v if host(k, v) else torch.from_numpy(v.view(np.uint8) if v.dtype in STRUCT else v).to(dev)) for k, v in f.items()}


def shared_rows(case, stride):
    """one descriptor array whose rows b * stride .. b * stride + m_cap are problem b's queries (overlapping windows); each problem's q_desc
    becomes its window, so that the oracle sees what the kernel reads"""
    D = np.ascontiguousarray(np.concatenate([p["q_desc"][:stride] for p in case.probs[:-1]] + [case.probs[-1]["q_desc"]]))
    for b, p in enumerate(case.probs):
        p["q_desc"] = D[b * stride: b * stride + case.m_cap].copy()
    return D


def run(case, mt, entry, t_counts=None, q_counts=None, stride=0, shared=None):
    """one call; returns (out_match, out_num, out_query_best) as numpy"""
    B, n_cap, m_cap = case.B, case.n_cap, case.m_cap
    f = case.fields()
    if t_counts is not None:
        f["t_counts"] = t_counts
    if q_counts is not None:
        f["q_counts"] = q_counts
    if stride:
        f["q_desc_stride"] = stride
        f["q_desc"] = shared
    kw = dict(case.kw)
    fuse = case.mode in FUSE
    if entry == "host":
        om, on, oq = np.full((B, n_cap), SENT, np.int32), np.full(B, SENT, np.int32), np.full((B, m_cap), SENT, np.int32)
        r = mt.match_host(case.mode, n_cap, m_cap, f, B=B, out_match=om, out_num=on, out_query_best=oq, **kw)
        return (None, None, r) if fuse else (r[0], r[1], None)
    import torch
    d = to_device(f)
    om = torch.full((B, n_cap), SENT, dtype=torch.int32, device="cuda:0")
    on = torch.full((B,), SENT, dtype=torch.int32, device="cuda:0")
    oq = torch.full((B, m_cap), SENT, dtype=torch.int32, device="cuda:0")
    if fuse:
        d["out_query_best"] = oq
    mt.match_device(case.mode, n_cap, m_cap, d, om, on, B=B, **kw)
    torch.cuda.synchronize()
    return (None, None, oq.cpu().numpy()) if fuse else (om.cpu().numpy(), on.cpu().numpy(), None)


def verify(case, res, t_counts=None, q_counts=None, what=""):
    om, on, oq = res
    total = 0
    for b in range(case.B):
        n = clamp(None if t_counts is None else t_counts[b], case.n_cap)
        m = clamp(None if q_counts is None else q_counts[b], case.m_cap)
        want = case.expect(b, n, m)
        if case.mode in FUSE:
            assert np.array_equal(oq[b, :m], want), (what, b, n, m)
            assert (oq[b, m:] == SENT).all(), (what, b, "slots beyond q_counts were written")
            total += int((want >= 0).sum())
        else:
            wm, wn = want
            assert on[b] == wn and np.array_equal(om[b, :n], wm), (what, b, n, m, int(on[b]), wn)
            assert (om[b, n:] == SENT).all(), (what, b, "slots beyond t_counts were written")
            total += wn
    return total


def check_case(case, want_plan, seed, stride=0):
    """the plan, then through one matcher: a host call at full counts (fills the staging slab), a ragged host call with sentinel-filled
    outputs, a ragged device call (optionally with overlapping query windows).  Returns the matches found."""
    assert case.plan() == want_plan
    rng = np.random.default_rng(seed)
    tc, qc = ragged(rng, case.B, case.n_cap, 0), ragged(rng, case.B, case.m_cap, 2)
    mt = plp.matcher(case.ratio, case.check)
    total = 0
    shared = shared_rows(case, stride) if stride else None
    if not stride:
        full = run(case, mt, "host")
        if case.mode in FUSE:
            assert (full[2] != SENT).all()
        else:
            assert (full[0] != SENT).all() and (full[1] != SENT).all()
        total += verify(case, full, what="host, full counts")
        total += verify(case, run(case, mt, "host", tc, qc), tc, qc, "host, ragged")
    dev = run(case, mt, "device", tc, qc, stride, shared)
    total += verify(case, dev, tc, qc, "device, ragged")
    return total


# ---------------------------------------------------------------------------------------------------- problems per mode
def T(p, n, k):
    return p[k][:n]


def point_probs(rng, B, n, m, stereo=True):
    out = []
    for b in range(B):
        t, q = MC.random_problem(rng, n, m, n_words=(0, 4, 12)[b % 3], stereo=stereo)
        out.append({**t, **q})
    return out


def landmarks_case(rng, B, n, m, grid):
    g6, margin, ratio = O.grid6(grid), 12.0, 0.8

    def oracle(p, n, m):
        return O.match_frame_and_landmarks(g6, T(p, n, "t_kps"), T(p, n, "t_desc"), T(p, n, "t_x_right"), T(p, n, "t_occupied"), SF, T(p, m, "q_valid"),
                                           T(p, m, "q_reproj"), T(p, m, "q_x_right"), T(p, m, "q_level"), T(p, m, "q_desc"), T(p, m, "q_has_obs"), margin, ratio)
    return Case(plp.MODE_LANDMARKS, point_probs(rng, B, n, m), n, m, oracle, ratio=ratio, margin=margin, scale_factors=SF, grid=grid)


LAST_FRAME_VARIANTS = ["direction", "marked", "keyframe", "sim3", "level_window_2"]


def last_frame_case(rng, B, n, m, grid, variant):
    g6, margin = O.grid6(grid), 15.0
    probs = point_probs(rng, B, n, m)
    ints, check, kw = {}, True, {}
    for b, p in enumerate(probs):
        p["q_angle"] = p["q_angle"].astype(np.float32)
        if variant in ("direction", "marked", "level_window_2"):
            p["directions"] = np.int32((b + b // 3) % 3)             # the motion direction differs between problems
    if variant == "marked":
        ints["flags"] = plp.FLAG_MARK_INVALIDATED
    if variant in ("keyframe", "sim3"):   # match_frame_and_keyframe / match_by_Sim3_transform: no stereo gate, every claim blocks
        for p in probs:
            for k in ("t_x_right", "q_x_right", "q_has_obs"):
                del p[k]
        ints["hamm_dist_thr"] = 50
    if variant == "sim3":
        ints.update(level_window=1, flags=plp.FLAG_UNSIGNED_LEVEL)
        check = False
    if variant == "level_window_2":
        ints["level_window"] = 2
        check = False

    def lf(p, n, m, direction, chk):
        return O.match_current_and_last(g6, T(p, n, "t_kps"), T(p, n, "t_desc"), T(p, n, "t_x_right"), T(p, n, "t_occupied"), SF, T(p, m, "q_valid"),
                                         T(p, m, "q_reproj"), T(p, m, "q_x_right"), T(p, m, "q_level"), T(p, m, "q_angle"), T(p, m, "q_desc"),
                                         T(p, m, "q_has_obs"), margin, direction, chk)

    def oracle(p, n, m):
        if variant == "direction":
            return lf(p, n, m, int(p["directions"]), True)
        if variant == "marked":   # -2 exactly where the orientation check removed a match
            want, wn = lf(p, n, m, int(p["directions"]), True)
            raw, _ = lf(p, n, m, int(p["directions"]), False)
            return np.where((raw >= 0) & (want < 0), -2, want).astype(np.int32), wn
        if variant == "level_window_2":   # [level - 1, level + 1] whatever the direction
            return lf(p, n, m, 0, False)
        pred = T(p, m, "q_level").astype(np.uint32)
        if variant == "keyframe":
            return O.match_frame_and_keyframe(g6, T(p, n, "t_kps"), T(p, n, "t_desc"), T(p, n, "t_occupied"), SF, T(p, m, "q_valid"), T(p, m, "q_reproj"),
                                              pred, T(p, m, "q_angle"), T(p, m, "q_desc"), margin, 50, True)
        return O.match_by_sim3(g6, T(p, n, "t_kps"), T(p, n, "t_desc"), T(p, n, "t_occupied"), SF, T(p, m, "q_valid"), T(p, m, "q_reproj"), pred,
                               T(p, m, "q_desc"), margin)
    return Case(plp.MODE_LAST_FRAME, probs, n, m, oracle, ratio=0.9, check=check, ints=ints, margin=margin, scale_factors=SF, grid=grid, **kw)


def brute_case(rng, B, n, m, check):
    probs = []
    for b in range(B):
        t, q = MC.random_problem(rng, n, m, n_words=(0, 5, 40)[b % 3])
        probs.append(dict(t_desc=t["t_desc"], t_angle=t["t_kps"]["angle"].copy(), q_desc=q["q_desc"], q_angle=q["q_angle"], q_valid=q["q_valid"]))

    def oracle(p, n, m):
        return O.brute_force_match(T(p, n, "t_desc"), T(p, n, "t_angle"), T(p, m, "q_desc"), T(p, m, "q_angle"), T(p, m, "q_valid"), 0.75, check)
    return Case(plp.MODE_BRUTE_FORCE, probs, n, m, oracle, ratio=0.75, check=check)


def bow_case(rng, B, n, m):
    probs = []
    for b in range(B):
        nodes = (40, 12, 3)[b % 3]
        t, q = MC.random_problem(rng, n, m, n_words=(0, 30, 4)[b % 3])
        t_node = (t["t_desc"][:, 0].astype(np.int32) * 7 + 3) % nodes
        q_node = (q["q_desc"][:, 0].astype(np.int32) * 7 + 3) % nodes
        o = np.argsort(q_node, kind="stable")
        probs.append(dict(t_desc=t["t_desc"], t_angle=t["t_kps"]["angle"].copy(), t_group=t_node, t_occupied=t["t_occupied"], q_desc=q["q_desc"][o],
                          q_angle=q["q_angle"][o], q_group=q_node[o].astype(np.int32), q_valid=q["q_valid"][o]))

    def oracle(p, n, m):
        return O.match_bow(T(p, m, "q_desc"), T(p, m, "q_angle"), T(p, m, "q_group"), T(p, m, "q_valid"), T(p, n, "t_desc"), T(p, n, "t_angle"),
                           T(p, n, "t_group"), T(p, n, "t_occupied"), 0.75, True)
    return Case(plp.MODE_BOW, probs, n, m, oracle, ratio=0.75, check=True)


def triangulation_case(rng, B, n, m, check):
    probs = []
    for b in range(B):
        tr = (0.3, 0.02, 0.05) if b % 2 == 0 else (-0.05, 0.25, 0.1 * (b % 5))   # E_12 and the epipole differ between problems
        (qd, qa, qn, q_has_lm, q_xr, q_oct, b1, td, ta, tn, t_has_lm, t_xr, b2, sf, E, ep) = MC.triangulation_problem(rng, n, m, (30, 10, 2)[b % 3],
                                                                                                                     (0, 25, 3)[b % 3], tr=tr)
        probs.append(dict(t_desc=td, t_angle=ta.copy(), t_group=tn.astype(np.int32), t_occupied=t_has_lm, t_x_right=t_xr, t_bearing=b2, q_desc=qd,
                          q_angle=qa, q_group=qn.astype(np.int32), q_valid=(1 - q_has_lm).astype(np.uint8), q_x_right=q_xr, q_level=q_oct, q_bearing=b1,
                          epipolar=np.concatenate([E, ep])))

    def oracle(p, n, m):
        E, ep = p["epipolar"][:9], p["epipolar"][9:]
        want, wn = O.match_for_triangulation(T(p, m, "q_desc"), T(p, m, "q_angle"), T(p, m, "q_group"), 1 - T(p, m, "q_valid"), T(p, m, "q_x_right"),
                                             T(p, m, "q_level"), T(p, m, "q_bearing"), T(p, n, "t_desc"), T(p, n, "t_angle"), T(p, n, "t_group"),
                                             T(p, n, "t_occupied"), T(p, n, "t_x_right"), T(p, n, "t_bearing"), SF, E, ep, check)
        want_t = np.full(n, -1, np.int32)
        sel = want >= 0
        want_t[want[sel]] = np.nonzero(sel)[0]
        return want_t, wn
    return Case(plp.MODE_TRIANGULATION, probs, n, m, oracle, ratio=0.9, check=check, scale_factors=SF)


def line_case(rng, B, n, m, mode):
    probs = []
    for b in range(B):
        t, q = MC.random_line_problem(rng, n, m, (0, 3, 1)[b % 3])
        p = {**t, **q}
        if mode == plp.MODE_LAST_FRAME_LINE:
            p["directions"] = np.int32(b % 3)
        probs.append(p)
    margin = 12.0
    if mode == plp.MODE_LANDMARKS_LINE:
        def oracle(p, n, m):
            return O.match_frame_and_landmarks_line(T(p, n, "t_kl"), T(p, n, "t_desc"), T(p, n, "t_kp_octave"), T(p, n, "t_occupied"), SF_LSD,
                                                    T(p, m, "q_valid"), T(p, m, "q_reproj"), T(p, m, "q_reproj2"), T(p, m, "q_level"), T(p, m, "q_desc"),
                                                    T(p, m, "q_has_obs"), margin, 0.8)
        return Case(mode, probs, n, m, oracle, ratio=0.8, margin=margin, scale_factors=SF_LSD)

    def oracle(p, n, m):
        xr = np.stack([T(p, n, "t_x_right"), T(p, n, "t_x_right2")], 1)
        return O.match_current_and_last_line(T(p, n, "t_kl"), T(p, n, "t_desc"), xr, T(p, n, "t_occupied"), SF_LSD, 1, T(p, m, "q_valid"), T(p, m, "q_reproj"),
                                             T(p, m, "q_reproj2"), T(p, m, "q_x_right"), T(p, m, "q_x_right2"), T(p, m, "q_level"), T(p, m, "q_desc"),
                                             T(p, m, "q_has_obs"), margin, int(p["directions"]), 1)
    return Case(mode, probs, n, m, oracle, ratio=0.9, check=True, ints=dict(is_rgbd=1, num_levels_lsd=1), margin=margin, scale_factors=SF_LSD)


FUSE_VARIANTS = ["chi2", "no_chi2", "signed_level"]


def fuse_case(rng, B, n, m, variant):
    g6, inv_sigma = O.grid6(G64), (1.0 / (SF * SF)).astype(np.float32)
    probs = []
    for b in range(B):
        t, q = MC.random_problem(rng, n, m, n_words=(0, 6)[b % 2], stereo=True)
        rd = q["q_reproj"].astype(np.float64) + rng.normal(0, 0.7, (m, 2))
        lvl = (rng.integers(0, 8, m) if variant == "chi2" else q["q_level"]).astype(np.int32)
        probs.append(dict(t_kps=t["t_kps"], t_desc=t["t_desc"], t_x_right=t["t_x_right"], q_valid=q["q_valid"], q_reproj_d=rd, q_x_right=q["q_x_right"],
                          q_level=lvl, q_desc=q["q_desc"]))
    ints = dict(inv_level_sigma_sq=inv_sigma) if variant == "chi2" else dict(inv_level_sigma_sq=np.ones(8, np.float32))
    if variant == "no_chi2":
        ints.update(flags=plp.FLAG_NO_CHI2, hamm_dist_thr=100)
    if variant == "signed_level":
        ints.update(flags=plp.FLAG_NO_CHI2 | plp.FLAG_SIGNED_LEVEL)
    margin = {"chi2": 3.0, "no_chi2": 7.5, "signed_level": 4.0}[variant]

    def oracle(p, n, m):
        pred = T(p, m, "q_level").astype(np.uint32)
        if variant == "chi2":
            return O.fuse_search(g6, T(p, n, "t_kps"), T(p, n, "t_desc"), T(p, n, "t_x_right"), SF, inv_sigma, T(p, m, "q_valid"), T(p, m, "q_reproj_d"),
                                 T(p, m, "q_x_right"), pred, T(p, m, "q_desc"), margin)
        thr, signed = (100, 0) if variant == "no_chi2" else (50, 1)
        return O.project_best(g6, T(p, n, "t_kps"), T(p, n, "t_desc"), SF, T(p, m, "q_valid"), T(p, m, "q_reproj_d"), pred, T(p, m, "q_desc"), margin, thr,
                              signed)
    return Case(plp.MODE_FUSE, probs, n, m, oracle, ints=ints, margin=margin, scale_factors=SF, grid=G64)


def fuse_line_case(rng, B, n, m):
    inv_sigma = np.array([1.0, 0.25], np.float32)
    probs = []
    for b in range(B):
        t, q = MC.random_line_problem(rng, n, m, (0, 4)[b % 2])
        sp = q["q_reproj"].astype(np.float64) + rng.normal(0, 0.2, (m, 2)); ep = q["q_reproj2"].astype(np.float64) + rng.normal(0, 0.2, (m, 2))
        probs.append(dict(t_kl=t["t_kl"], t_desc=t["t_desc"], q_valid=q["q_valid"], q_reproj_d=sp, q_reproj2_d=ep, q_level=q["q_level"], q_desc=q["q_desc"]))

    def oracle(p, n, m):
        return O.fuse_search_line(T(p, n, "t_kl"), T(p, n, "t_desc"), SF_LSD, inv_sigma, T(p, m, "q_valid"), T(p, m, "q_reproj_d"), T(p, m, "q_reproj2_d"),
                                  T(p, m, "q_level").astype(np.uint32), T(p, m, "q_desc"), 6.0)
    return Case(plp.MODE_FUSE_LINE, probs, n, m, oracle, ints=dict(inv_level_sigma_sq=inv_sigma), margin=6.0, scale_factors=SF_LSD)


# ---------------------------------------------------------------------------------------------------- a. + b. the path matrix, ragged
CELLS_1, CELLS_64 = ("cells", "grid", 32, "sorted"), ("cells", "grid", 512, "sorted")
LANES, TOPK = ("lanes", "point", 0, "generic"), ("topk", "point", 0, "generic")
# (label, grid, B, n_cap, m_cap, plan): the cells path with 32 and 512 queries per workgroup, then the generic paths on a 256-column grid
WINDOWED_PATHS = [("cells32", G64, 6, 700, 900, CELLS_1), ("cells512", G64, 64, 300, 400, CELLS_64),
                  ("lanes", G256, 66, 400, 500, LANES), ("topk", G256, 6, 700, 900, TOPK)]


@pytest.mark.parametrize("path", WINDOWED_PATHS, ids=lambda p: p[0])
def test_landmarks_every_path(path):
    label, grid, B, n, m, plan = path
    rng = np.random.default_rng(1000 + B)
    assert check_case(landmarks_case(rng, B, n, m, grid), plan, 1) > 0


@pytest.mark.parametrize("variant", LAST_FRAME_VARIANTS)
@pytest.mark.parametrize("path", [p for p in WINDOWED_PATHS if p[0] != "cells512"], ids=lambda p: p[0])
def test_last_frame_variants_every_path(path, variant):
    label, grid, B, n, m, plan = path
    rng = np.random.default_rng(2000 + B + LAST_FRAME_VARIANTS.index(variant))
    assert check_case(last_frame_case(rng, B, n, m, grid, variant), plan, 2) > 0


def test_last_frame_batch_of_64_on_the_cells_path():
    rng = np.random.default_rng(2100)
    assert check_case(last_frame_case(rng, 64, 300, 400, G64, "direction"), CELLS_64, 3) > 0


def test_windowed_frames_beyond_the_lds_staging():
    """more targets than the cells path can stage (16 B each with t_x_right): one wave per query on a 64 x 48 grid, several problems"""
    rng = np.random.default_rng(2200)
    grid = plp.make_grid(1241, 376)
    probs = []
    for b in range(3):
        t, q = MC.random_problem(rng, 3700, 1500, n_words=(0, 12)[b % 2], cols=1241, rows=376, stereo=True)
        probs.append({**t, **q})
    g6 = O.grid6(grid)

    def oracle(p, n, m):
        return O.match_frame_and_landmarks(g6, T(p, n, "t_kps"), T(p, n, "t_desc"), T(p, n, "t_x_right"), T(p, n, "t_occupied"), SF, T(p, m, "q_valid"),
                                           T(p, m, "q_reproj"), T(p, m, "q_x_right"), T(p, m, "q_level"), T(p, m, "q_desc"), T(p, m, "q_has_obs"), 12.0, 0.8)
    assert check_case(Case(plp.MODE_LANDMARKS, probs, 3700, 1500, oracle, margin=12.0, scale_factors=SF, grid=grid), TOPK, 4) > 0


@pytest.mark.parametrize("n_cap,plan", [(2048, ("lds", "point", 128, "generic")), (2049, TOPK), (4000, TOPK)])
def test_brute_force_every_path(n_cap, plan):
    rng = np.random.default_rng(3000 + n_cap)
    assert check_case(brute_case(rng, 6, n_cap, 700, check=n_cap != 2049), plan, 5) > 0


@pytest.mark.parametrize("B,n,m,kernel", [(66, 300, 350, "lanes"), (6, 900, 800, "topk")])
def test_bow_every_path(B, n, m, kernel):
    rng = np.random.default_rng(4000 + B)
    assert check_case(bow_case(rng, B, n, m), (kernel, "group", 0, "generic"), 6) > 0


@pytest.mark.parametrize("B,n,m,kernel", [(64, 400, 300, "lanes"), (7, 900, 800, "topk")])
@pytest.mark.parametrize("check", [True, False])
def test_triangulation_every_path(B, n, m, kernel, check):
    rng = np.random.default_rng(5000 + B + check)
    assert check_case(triangulation_case(rng, B, n, m, check), (kernel, "group", 0, "generic"), 7) > 0


@pytest.mark.parametrize("mode", [plp.MODE_LANDMARKS_LINE, plp.MODE_LAST_FRAME_LINE])
@pytest.mark.parametrize("B,n,m,kernel", [(70, 128, 200, "lanes"), (6, 600, 500, "topk")])
def test_line_modes_every_path(mode, B, n, m, kernel):
    rng = np.random.default_rng(6000 + B + mode)
    assert check_case(line_case(rng, B, n, m, mode), (kernel, "line", 0, "generic"), 8) > 0


@pytest.mark.parametrize("variant", FUSE_VARIANTS)
def test_fuse_batched(variant):
    rng = np.random.default_rng(7000 + FUSE_VARIANTS.index(variant))
    assert check_case(fuse_case(rng, 6, 900, 700, variant), ("fuse", "any", 0, None), 9) > 0


def test_fuse_line_batched():
    rng = np.random.default_rng(7100)
    assert check_case(fuse_line_case(rng, 6, 300, 400), ("fuse", "any", 0, None), 10) > 0


# ---------------------------------------------------------------------------------------------------- d. overlapping query windows
def test_overlapping_query_windows_on_the_device_entry():
    """q_desc_stride < m_cap: problem b's queries are rows b * stride .. b * stride + m_cap of one shared descriptor array"""
    rng = np.random.default_rng(8000)
    assert check_case(brute_case(rng, 5, 800, 600, True), ("lds", "point", 128, "generic"), 11, stride=250) > 0
    assert check_case(bow_case(rng, 66, 300, 350), ("lanes", "group", 0, "generic"), 12, stride=200) > 0
    assert check_case(bow_case(rng, 5, 700, 600), ("topk", "group", 0, "generic"), 13, stride=100) > 0
    assert check_case(fuse_case(rng, 5, 900, 700, "chi2"), ("fuse", "any", 0, None), 14, stride=350) > 0


# ---------------------------------------------------------------------------------------------------- c. crowded windows
def graded(rng, k, width=128):
    """a base descriptor and k targets at Hamming distances 0, 1, .., k-1 from it (nested bit sets inside the first `width` bits)"""
    base = rng.integers(0, 256, 32, dtype=np.uint8)
    bits = rng.permutation(width)
    t = np.repeat(base[None], k, 0)
    for i in range(k):
        for bit in bits[:i]:
            t[i, bit >> 3] ^= np.uint8(1 << (bit & 7))
    return base, t


def far(base, extra):
    """base moved by `extra` bits outside the graded bits (128..255): `extra` farther from every graded target"""
    d = base.copy()
    for bit in range(128, 128 + extra):
        d[bit >> 3] ^= np.uint8(1 << (bit & 7))
    return d


def crowd_queries(base, n_plain, probes):
    """n_plain queries that each take the nearest free target, with probes inserted after the given number of plain queries:
    probe = (after, extra distance)"""
    rows, at = [], sorted(probes)
    for i in range(n_plain + 1):
        rows += [far(base, e) for a, e in at if a == i]
        if i < n_plain:
            rows.append(base.copy())
    return np.stack(rows)


def point_crowd(rng, k, q_desc, box, reproj):
    x0, y0, x1, y1 = box
    kps = np.zeros(k, O.KP_DTYPE)
    kps["x"], kps["y"] = rng.uniform(x0, x1, k).astype(np.float32), rng.uniform(y0, y1, k).astype(np.float32)
    kps["angle"] = rng.uniform(0, 360, k).astype(np.float32)
    m = len(q_desc)
    return dict(t_kps=kps, t_occupied=np.zeros(k, np.uint8), q_valid=np.ones(m, np.uint8), q_reproj=np.tile(np.float32(reproj), (m, 1)),
                q_level=np.zeros(m, np.int32), q_angle=np.full(m, 10.0, np.float32), q_desc=q_desc, q_has_obs=np.ones(m, np.uint8))


CELL_BOX = {"sorted": ((100.5, 100.5, 109.5, 109.5), (105.0, 105.0), G64), "generic": ((100.2, 98.0, 102.3, 112.0), (101.0, 105.0), G256)}


def crowd_case(rng, mode, path, k, n_plain, probes, B=2):
    """B copies (different positions, same structure) of one crowded window: k targets in one grid cell (one BoW node), graded distances"""
    probs = []
    for b in range(B):
        base, td = graded(rng, k)
        qd = crowd_queries(base, n_plain, probes)
        m = len(qd)
        if mode in (plp.MODE_LANDMARKS, plp.MODE_LAST_FRAME):
            box, reproj, grid = CELL_BOX[path]
            p = point_crowd(rng, k, qd, box, reproj)
            p["t_desc"] = td
        elif mode in (plp.MODE_BRUTE_FORCE, plp.MODE_BOW):
            p = dict(t_desc=td, t_angle=np.full(k, 5.0, np.float32), q_desc=qd, q_angle=np.full(m, 10.0, np.float32), q_valid=np.ones(m, np.uint8))
            if mode == plp.MODE_BOW:
                p.update(t_group=np.zeros(k, np.int32), q_group=np.zeros(m, np.int32), t_occupied=np.zeros(k, np.uint8))
        elif mode == plp.MODE_TRIANGULATION:
            # pairs of targets at EQUAL distances (the later index must win), all on the epipolar plane of one 3-D point
            td = np.repeat(td[: (k + 1) // 2], 2, 0)[:k].copy()
            for i in range(1, k, 2):   # the second of a pair: the same distance from base, other bits
                td[i] = base
                for bit in rng.permutation(np.arange(128, 256))[:np.unpackbits(td[i - 1] ^ base).sum()]:
                    td[i, bit >> 3] ^= np.uint8(1 << (bit & 7))
            qd = crowd_queries(base, n_plain, [])
            m = len(qd)
            tr = np.array([0.3, 0.02, 0.05]) if b % 2 == 0 else np.array([-0.1, 0.2, 0.05])
            E = np.array([[0, -tr[2], tr[1]], [tr[2], 0, -tr[0]], [-tr[1], tr[0], 0]], np.float64)
            P = np.array([0.5 + 0.1 * b, 0.3, 5.0])
            b1 = P / np.linalg.norm(P); b2 = (P - tr) / np.linalg.norm(P - tr)
            p = dict(t_desc=td, t_angle=np.full(k, 5.0, np.float32), t_group=np.zeros(k, np.int32), t_occupied=np.zeros(k, np.uint8),
                     t_x_right=np.full(k, -1, np.float32), t_bearing=np.tile(b2, (k, 1)), q_desc=qd, q_angle=np.full(m, 10.0, np.float32),
                     q_group=np.zeros(m, np.int32), q_valid=np.ones(m, np.uint8), q_x_right=np.full(m, -1, np.float32), q_level=np.zeros(m, np.int32),
                     q_bearing=np.tile(b1, (m, 1)), epipolar=np.concatenate([E.ravel(), -tr / np.linalg.norm(tr)]))
        elif mode == plp.MODE_LANDMARKS_LINE:
            kl = np.zeros(k, O.KL_DTYPE)
            kl["startPointX"] = 100 + rng.uniform(-0.5, 0.5, k); kl["startPointY"] = 100 + rng.uniform(-0.5, 0.5, k)
            kl["endPointX"] = 200 + rng.uniform(-0.5, 0.5, k); kl["endPointY"] = 150 + rng.uniform(-0.5, 0.5, k)
            p = dict(t_kl=kl, t_desc=td, t_kp_octave=np.zeros(k, np.int32), t_occupied=np.zeros(k, np.uint8), q_valid=np.ones(m, np.uint8),
                     q_reproj=np.tile(np.float32([100, 100]), (m, 1)), q_reproj2=np.tile(np.float32([200, 150]), (m, 1)), q_level=np.zeros(m, np.int32),
                     q_desc=qd, q_has_obs=np.ones(m, np.uint8))
        probs.append(p)
    n, m = k, len(probs[0]["q_desc"])
    if mode == plp.MODE_LANDMARKS:
        grid = CELL_BOX[path][2]; g6 = O.grid6(grid)

        def oracle(p, n, m):
            return O.match_frame_and_landmarks(g6, T(p, n, "t_kps"), T(p, n, "t_desc"), np.full(n, -1, np.float32), T(p, n, "t_occupied"), SF,
                                               T(p, m, "q_valid"), T(p, m, "q_reproj"), np.full(m, -1, np.float32), T(p, m, "q_level"), T(p, m, "q_desc"),
                                               T(p, m, "q_has_obs"), 8.0, 1.0)
        return Case(mode, probs, n, m, oracle, ratio=1.0, margin=8.0, scale_factors=SF, grid=grid)
    if mode == plp.MODE_LAST_FRAME:
        grid = CELL_BOX[path][2]; g6 = O.grid6(grid)

        def oracle(p, n, m):
            return O.match_current_and_last(g6, T(p, n, "t_kps"), T(p, n, "t_desc"), np.full(n, -1, np.float32), T(p, n, "t_occupied"), SF,
                                            T(p, m, "q_valid"), T(p, m, "q_reproj"), np.full(m, -1, np.float32), T(p, m, "q_level"), T(p, m, "q_angle"),
                                            T(p, m, "q_desc"), T(p, m, "q_has_obs"), 8.0, 0, False)
        return Case(mode, probs, n, m, oracle, ratio=1.0, margin=8.0, scale_factors=SF, grid=grid)
    if mode == plp.MODE_BRUTE_FORCE:
        def oracle(p, n, m):
            return O.brute_force_match(T(p, n, "t_desc"), T(p, n, "t_angle"), T(p, m, "q_desc"), T(p, m, "q_angle"), T(p, m, "q_valid"), 1.0, False)
        return Case(mode, probs, n, m, oracle, ratio=1.0)
    if mode == plp.MODE_BOW:
        def oracle(p, n, m):
            return O.match_bow(T(p, m, "q_desc"), T(p, m, "q_angle"), T(p, m, "q_group"), T(p, m, "q_valid"), T(p, n, "t_desc"), T(p, n, "t_angle"),
                               T(p, n, "t_group"), T(p, n, "t_occupied"), 1.0, False)
        return Case(mode, probs, n, m, oracle, ratio=1.0)
    if mode == plp.MODE_TRIANGULATION:
        def oracle(p, n, m):
            want, wn = O.match_for_triangulation(T(p, m, "q_desc"), T(p, m, "q_angle"), T(p, m, "q_group"), 1 - T(p, m, "q_valid"), T(p, m, "q_x_right"),
                                                 T(p, m, "q_level"), T(p, m, "q_bearing"), T(p, n, "t_desc"), T(p, n, "t_angle"), T(p, n, "t_group"),
                                                 T(p, n, "t_occupied"), T(p, n, "t_x_right"), T(p, n, "t_bearing"), SF, p["epipolar"][:9], p["epipolar"][9:],
                                                 False)
            want_t = np.full(n, -1, np.int32)
            sel = want >= 0
            want_t[want[sel]] = np.nonzero(sel)[0]
            return want_t, wn
        return Case(mode, probs, n, m, oracle, ratio=1.0, scale_factors=SF)

    def oracle(p, n, m):
        return O.match_frame_and_landmarks_line(T(p, n, "t_kl"), T(p, n, "t_desc"), T(p, n, "t_kp_octave"), T(p, n, "t_occupied"), SF_LSD,
                                                T(p, m, "q_valid"), T(p, m, "q_reproj"), T(p, m, "q_reproj2"), T(p, m, "q_level"), T(p, m, "q_desc"),
                                                T(p, m, "q_has_obs"), 6.0, 1.0)
    return Case(mode, probs, n, m, oracle, ratio=1.0, margin=6.0, scale_factors=SF_LSD)


def run_crowd(case, want_plan):
    """full counts through the host entry on a fresh matcher: the oracle's answer and the number of exact rescans"""
    assert case.plan() == want_plan
    mt = plp.matcher(case.ratio, case.check)
    before = int(mt.debug_counters()[0])
    res = run(case, mt, "host")
    verify(case, res, what="crowd")
    return res, int(mt.debug_counters()[0]) - before


def claimed(res, b):
    return int((res[0][b] >= 0).sum())


# (mode, path, plan): one per resolve instantiation and list length (16 on the cells path, 8 elsewhere)
CROWD_RESOLVES = [(plp.MODE_LANDMARKS, "sorted", CELLS_1, 16), (plp.MODE_LAST_FRAME, "sorted", CELLS_1, 16),
                  (plp.MODE_LANDMARKS, "generic", TOPK, 8), (plp.MODE_LAST_FRAME, "generic", TOPK, 8),
                  (plp.MODE_BRUTE_FORCE, None, ("lds", "point", 128, "generic"), 8), (plp.MODE_BOW, None, ("topk", "group", 0, "generic"), 8),
                  (plp.MODE_LANDMARKS_LINE, None, ("topk", "line", 0, "generic"), 8)]


@pytest.mark.parametrize("mode,path,plan,klen", CROWD_RESOLVES, ids=lambda v: str(v))
def test_crowded_window_lists_that_just_suffice(mode, path, plan, klen):
    """klen plain queries against 40 targets: the i-th takes the i-th nearest.  The last one's list (candidates 9-16 on the cells path come
    from its second list) holds one free entry: the d8 shortcut decides it -- for the landmark matchers the ratio test against d8, for the
    others the Lowe test against d8 -- and no query needs the exact rescan"""
    rng = np.random.default_rng(9000 + mode)
    res, rescans = run_crowd(crowd_case(rng, mode, path, 40, klen, []), plan)
    assert all(claimed(res, b) == klen for b in range(2))
    assert rescans == 0


@pytest.mark.parametrize("mode,path,plan,klen", CROWD_RESOLVES, ids=lambda v: str(v))
def test_crowded_window_lists_that_run_dry(mode, path, plan, klen):
    """30 plain queries against 40 targets: from the (klen + 1)-th on every list entry is taken and only the exact rescan finds the answer.
    Probes (a query 101 bits farther from every target, after klen - 1 and after 20 plain queries): nothing under the threshold is left
    (d8 > 100, or the one free entry is over it) -- no claim, no rescan needed"""
    rng = np.random.default_rng(9100 + mode)
    probes = [(klen - 1, 101), (20, 101)] if mode in (plp.MODE_LANDMARKS, plp.MODE_LAST_FRAME, plp.MODE_LANDMARKS_LINE) else [(klen - 1, 51), (20, 51)]
    res, rescans = run_crowd(crowd_case(rng, mode, path, 40, 30, probes), plan)
    assert all(claimed(res, b) == 30 for b in range(2))
    assert rescans >= 2 * (30 - klen)


def test_crowded_triangulation_equal_distances_inside_the_rescan():
    """pairs of targets at equal distances (the reference keeps the LATER one, robust.cc:124), 30 queries: the rescans pick among equals"""
    rng = np.random.default_rng(9200)
    case = crowd_case(rng, plp.MODE_TRIANGULATION, None, 40, 30, [])
    res, rescans = run_crowd(case, ("topk", "group", 0, "generic"))
    assert all(claimed(res, b) == 30 for b in range(2))
    assert rescans > 0
    # lanes path: the same crowd in a batch of 64
    big = Case(case.mode, case.probs * 32, case.n_cap, case.m_cap, case.oracle, ratio=1.0, scale_factors=SF)
    res, rescans = run_crowd(big, ("lanes", "group", 0, "generic"))
    assert rescans > 0


def test_crowded_windows_on_the_lanes_paths():
    """the crowds of the point and line matchers in batches of 64: one lane per query, then the generic resolve with its rescans"""
    rng = np.random.default_rng(9300)
    for mode, plan in ((plp.MODE_LANDMARKS, LANES), (plp.MODE_LANDMARKS_LINE, ("lanes", "line", 0, "generic")), (plp.MODE_BOW, ("lanes", "group", 0, "generic"))):
        case = crowd_case(rng, mode, "generic", 40, 30, [], B=64)
        res, rescans = run_crowd(case, plan)
        assert all(claimed(res, b) == 30 for b in range(64)) and rescans >= 64 * 22


# ---------------------------------------------------------------------------------------------------- f. LBD 1-NN batched, Hamming sizes
def test_lbd_match_1nn_device_batched_ragged():
    import torch
    rng = np.random.default_rng(9400)
    B, nq_cap, nt_cap = 7, 150, 170
    vocab = rng.integers(0, 256, (5, 32), dtype=np.uint8)
    q = np.stack([vocab[rng.integers(0, 5, nq_cap)] ^ (rng.uniform(size=(nq_cap, 32)) < 0.02).astype(np.uint8) for _ in range(B)])
    t = np.stack([vocab[rng.integers(0, 5, nt_cap)] ^ (rng.uniform(size=(nt_cap, 32)) < 0.02).astype(np.uint8) for _ in range(B)])
    qc, tc = ragged(rng, B, nq_cap, 0), ragged(rng, B, nt_cap, 3)
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in dict(q=q, t=t, qc=qc, tc=tc).items()}
    idx = torch.full((B, nq_cap), SENT, dtype=torch.int32, device="cuda:0"); dist = torch.full((B, nq_cap), SENT, dtype=torch.int32, device="cuda:0")
    mt = plp.matcher()
    st = torch.cuda.current_stream().cuda_stream
    plp._check(plp.lib().plp_lbd_match_1nn_device(mt._h, d["q"].data_ptr(), d["qc"].data_ptr(), nq_cap, d["t"].data_ptr(), d["tc"].data_ptr(), nt_cap, B,
                                                   idx.data_ptr(), dist.data_ptr(), C.c_void_p(st)))
    torch.cuda.synchronize()
    idx, dist = idx.cpu().numpy(), dist.cpu().numpy()
    for b in range(B):
        nq, nt = clamp(qc[b], nq_cap), clamp(tc[b], nt_cap)
        assert (idx[b, nq:] == SENT).all() and (dist[b, nq:] == SENT).all(), b
        if nq == 0:
            continue
        if nt == 0:   # nothing to match: every query reports none
            assert (idx[b, :nq] == -1).all() and (dist[b, :nq] == 256).all(), b
            continue
        wi, wd = O.lbd_match_1nn(q[b, :nq], t[b, :nt])
        assert np.array_equal(idx[b, :nq], wi) and np.array_equal(dist[b, :nq], wd), b


@pytest.mark.parametrize("nq,nt", [(1, 1), (63, 65), (65, 63), (130, 1), (1, 130), (63, 130), (130, 65)])
def test_hamming_matrix_sizes_off_the_tile(nq, nt):
    rng = np.random.default_rng(nq * 1000 + nt)
    q = rng.integers(0, 256, (nq, 32), dtype=np.uint8); t = rng.integers(0, 256, (nt, 32), dtype=np.uint8)
    want = np.unpackbits(q[:, None, :] ^ t[None, :, :], axis=2).sum(2)
    assert np.array_equal(plp.matcher().hamming_matrix(q, t), want)
    import torch
    dq, dt = torch.from_numpy(q).cuda(), torch.from_numpy(t).cuda()
    out = torch.full((nq * nt + 64,), 0x3B3B, dtype=torch.int16, device="cuda:0")
    mt = plp.matcher()
    plp._check(plp.lib().plp_hamming_matrix_device(mt._h, dq.data_ptr(), nq, dt.data_ptr(), nt, out.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(np.uint16)
    assert np.array_equal(got[: nq * nt].reshape(nq, nt), want)
    assert (got[nq * nt:] == 0x3B3B).all()   # nothing past the matrix
