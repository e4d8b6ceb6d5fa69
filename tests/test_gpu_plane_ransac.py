"""Planar_Mapping_module's RANSAC and refine_points on the device (plp_plane_ransac_device / _host, plp_plane_refine_points_*,
csrc/plane_kernels.hip) against the CPU build of the same header (plp.model_plane_ransac, which tests/test_plane_ransac_cpu.py holds bit for
bit to the restatement tests/plane_ransac_ref.py): every output bit for bit on sentinel-filled arrays, at the smallest
shapes at which the kernels can go wrong -- eligible counts at points_per_ransac and one below, around the wave (64) and the 256-slot round
of the compaction, 8192 slots, holes that move ranks off slots, ragged problems with rows of count 0, iteration counts around the
workgroup's four waves, both modes, caller's and drawn samples, ranks out of range, a NaN position, NULL optionals and two calls back to
back on one stream."""
import numpy as np
import pytest

import plane_ransac_ref as PR
import plane_ransac_scene as PS
from plp import plp

pytestmark = pytest.mark.gpu
OPTIONAL = ("hyp_residual", "hyp_inliers", "hyp_error")
WAVES = 4                                                # waves of k_plane_hypotheses' workgroup: hypotheses are dealt to them


@pytest.fixture(scope="module")
def mt():
    return plp.matcher()


def sentinels(P, n_cap, iters):
    return {k: np.full((P,) + shape(n_cap, iters), PR.SENTINEL[k], dt) for k, (shape, dt, _) in plp.PLANE_RANSAC_OUTPUTS.items()}


def same_bits(a, b, nan_ok=False):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if nan_ok and a.dtype.kind == "f":                   # a NaN's sign and payload are not part of the contract
        return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def enqueue_device(mt, problems, a, skip_optional=False, stream=None):
    """plp_plane_ransac_device on sentinel-filled device outputs; returns the output tensors (nothing is synchronised)"""
    import torch
    q = problems[0]
    P, n_cap = a["flags"].shape
    d = lambda v: None if v is None else torch.from_numpy(np.ascontiguousarray(v).copy()).cuda()
    o = {k: d(v) for k, v in sentinels(P, n_cap, q["iters"]).items()}
    passed = {k: v for k, v in o.items() if not (skip_optional and k in OPTIONAL)}
    dev = {k: d(a[k]) for k in a}
    mt.plane_ransac_device(q["mode"], P, n_cap, dev["pos_w"], dev["flags"], dev["dist_thresh"], dev["error_thresh"], passed,
                           points_per_ransac=q["points_per_ransac"], iters=q["iters"], best_error_in=dev["best_error_in"], equation_in=dev["equation_in"],
                           samples=dev["samples"], m_cap=0 if a["samples"] is None else a["samples"].shape[2], seed=q["seed"],
                           counts=None if skip_optional else dev["counts"], stream=stream)
    return o, dev


def check(mt, problems, n_cap=None, host=True, skip_optional=False, nan_ok=False):
    import torch
    for q in problems:
        q["seed"] = problems[0]["seed"]
    a = PS.pack(problems, n_cap)
    P, n_cap = a["flags"].shape
    q = problems[0]
    kw = PS.call_kwargs(problems, a)
    if skip_optional:
        kw["counts"] = None
    pos = (q["mode"], a["pos_w"], a["flags"], a["dist_thresh"], a["error_thresh"])
    want = plp.model_plane_ransac(*pos, out=sentinels(P, n_cap, q["iters"]), **kw)
    o, _ = enqueue_device(mt, problems, a, skip_optional)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in o.items()}
    for k in want:
        if skip_optional and k in OPTIONAL:
            assert (got[k] == PR.SENTINEL[k]).all(), ("an output that was not passed was written", k)
        else:
            assert same_bits(got[k], want[k], nan_ok), ("device", k, got[k], want[k])
    if host:
        h = mt.plane_ransac(*pos, out=sentinels(P, n_cap, q["iters"]), **kw)
        for k in want:
            assert same_bits(h[k], want[k], nan_ok), ("host entry", k, h[k], want[k])
    return want


# eligible counts: points_per_ransac and one below, the wave edge, the 256-slot round of the compaction; the holes move ranks off slots
@pytest.mark.parametrize("mode", [PR.CREATE, PR.UPDATE])
@pytest.mark.parametrize("n_eligible", [17, 18, 63, 64, 65, 255, 256, 257])
def test_eligible_counts_around_every_edge(mt, mode, n_eligible):
    erased, unowned = 5, (4 if mode == PR.UPDATE else 0)
    q = PS.problem(200 + n_eligible, n_eligible + erased + unowned, mode=mode, outliers=0.05, erased=erased, unowned=unowned, iters=6)
    want = check(mt, [q])
    assert int(want["last_iter"][0]) >= 0 and int(want["hyp_inliers"][0].max()) > 0


def test_8192_slots_both_modes(mt):
    for mode, iters in ((PR.CREATE, 5), (PR.UPDATE, 2)):
        q = PS.problem(300 + mode, 8192, mode=mode, outliers=0.02, erased=300, unowned=200 if mode == PR.UPDATE else 0, iters=iters)
        want = check(mt, [q], host=mode == PR.CREATE)
        assert int(want["status"][0]) == PR.OK and int(want["num_inliers"][0]) > 7000


@pytest.mark.parametrize("P", [1, 3, 130])
def test_ragged_problems_with_empty_rows_between_full_ones(mt, P):
    sizes = [(90, 4), (0, 0), (150, 0), (17, 0), (40, 40), (65, 1), (10, 0)]
    qs = [PS.problem(400 + p, *sizes[p % len(sizes)][:1], erased=sizes[p % len(sizes)][1], outliers=0.05, iters=5) for p in range(P)]
    want = check(mt, qs, n_cap=160, host=P <= 3)
    if P >= 7:
        assert {PR.OK, PR.TOO_FEW_POINTS, PR.NO_ELIGIBLE} <= set(int(s) for s in want["status"])
        assert (want["flags"][6::7] == PR.FLAG_GATED).all()


# 1; the reference's 50; one more than the workgroup's waves; a multiple of the waves plus one
@pytest.mark.parametrize("iters", [1, 50, WAVES + 1, 3 * WAVES + 1])
def test_iteration_counts_around_the_waves(mt, iters):
    q = PS.problem(500 + iters, 140, outliers=0.2, erased=6, iters=iters, error_thresh=1e-9)   # no break: the last iteration decides the outputs
    want = check(mt, [q])
    assert int(want["last_iter"][0]) == iters - 1


def test_callers_samples_plans_and_ranks_out_of_range(mt):
    for name in ("break_mid", "never", "best_not_last"):
        q = dict(PS.scenes()[name][0])
        want = check(mt, [q])
        assert (want["hyp_residual"][0] == PR.DBL_MAX).any() == (name != "best_not_last")
    for name in ("u_ok", "u_last_dirty", "u_need_refinement", "u_above"):
        check(mt, [dict(PS.scenes()[name][0])])
    q = PS.problem(600, 80, plan="xxxx", iters=4)                                    # no hypothesis has a valid sample
    want = check(mt, [q])
    assert int(want["status"][0]) == PR.NOT_FOUND and (want["equation"][0] == 0.0).all() and want["best_error"][0] == PR.DBL_MAX


def test_nan_in_one_position(mt):
    q = PS.problem(700, 100, outliers=0.05, plan="cccc", iters=4)
    live = np.flatnonzero((q["flags"] & PR.LM_ERASED) == 0)
    q["pos_w"][live[int(q["samples"][1, 3])], 1] = np.nan                             # a sampled point of iteration 1
    check(mt, [q], nan_ok=True)


def test_null_optionals_p_zero_and_two_calls_on_one_stream(mt):
    import torch
    q = PS.problem(800, 120, outliers=0.1, iters=7)
    check(mt, [q], skip_optional=True, host=False)                                    # hyp_* and counts NULL
    a = PS.pack([q])
    before = sentinels(1, 120, 7)
    empty = {k: v[:0] for k, v in before.items()}
    mt.plane_ransac(PR.CREATE, a["pos_w"][:0], a["flags"][:0], [], [], iters=7, out=empty)            # P = 0
    d = lambda v: torch.from_numpy(v.copy()).cuda()
    o = {k: d(v) for k, v in before.items()}
    mt.plane_ransac_device(PR.CREATE, 0, 120, d(a["pos_w"]), d(a["flags"]), d(a["dist_thresh"]), d(a["error_thresh"]), o, iters=7)
    mt.plane_ransac_device(PR.CREATE, 1, 0, d(a["pos_w"]), d(a["flags"]), d(a["dist_thresh"]), d(a["error_thresh"]), o, iters=7)
    torch.cuda.synchronize()
    assert all(same_bits(o[k].cpu().numpy(), before[k]) for k in o), "P == 0 or n_cap == 0 wrote an output"
    # two calls back to back on one stream, the second with more problems, slots and iterations: the context's buffer is reused and regrown
    q1 = [PS.problem(810 + p, 70, outliers=0.05, iters=3) for p in range(2)]
    q2 = [PS.problem(820 + p, 300, outliers=0.05, erased=9, iters=9) for p in range(5)]
    for q in q1 + q2:
        q["seed"] = 5
    a1, a2 = PS.pack(q1), PS.pack(q2, 333)
    w1 = plp.model_plane_ransac(PR.CREATE, a1["pos_w"], a1["flags"], a1["dist_thresh"], a1["error_thresh"], out=sentinels(2, 70, 3), **PS.call_kwargs(q1, a1))
    w2 = plp.model_plane_ransac(PR.CREATE, a2["pos_w"], a2["flags"], a2["dist_thresh"], a2["error_thresh"], out=sentinels(5, 333, 9), **PS.call_kwargs(q2, a2))
    o1, keep1 = enqueue_device(mt, q1, a1)
    o2, keep2 = enqueue_device(mt, q2, a2)
    o3, keep3 = enqueue_device(mt, q1, a1)
    torch.cuda.synchronize()
    for o, w in ((o1, w1), (o2, w2), (o3, w1)):
        for k in w:
            assert same_bits(o[k].cpu().numpy(), w[k]), k


@pytest.mark.parametrize("M", [1, 64, 65, 4097])
def test_refine_points_equals_its_restatement(mt, M):
    import torch
    sc = PS.refine_scene(900 + M, M)
    want_pos, want_ch = PR.refine_points(**sc)
    assert want_ch.sum() > 0 or M == 1
    for fn in (plp.model_plane_refine_points, mt.plane_refine_points):
        pos, ch = fn(**sc)
        assert same_bits(ch, want_ch) and np.array_equal(pos, want_pos, equal_nan=True) and same_bits(pos[want_ch == 1], want_pos[want_ch == 1])
    d = lambda v: torch.from_numpy(np.ascontiguousarray(v).copy()).cuda()
    pos, ch = d(sc["pos_w"]), d(np.full(M, 0xEE, np.uint8))
    mt.plane_refine_points_device(M, len(sc["equation"]), pos, d(sc["lm_plane"]), d(sc["flags"]), d(sc["equation"]), d(sc["active"]),
                                  d(np.array([sc["dist_thresh"]])), ch)
    torch.cuda.synchronize()
    assert same_bits(ch.cpu().numpy(), want_ch) and same_bits(pos.cpu().numpy(), np.where(want_ch[:, None] == 1, want_pos, sc["pos_w"]))
