"""solve::essential_solver on the device (plp_essential_ransac_device / _host, csrc/essential_kernels.hip) against the CPU build of the same
header (plp.model_essential_ransac, which tests/test_two_view_cpu.py holds bit for bit to the restatement tests/two_view_ref.py; DESIGN.md
section 5, D24): every output bit for bit on sentinel-filled arrays, at the smallest shapes at which the kernels can go wrong -- numbers of
matches around the sample size (8), the wave (64), the compaction chunk and the LDS tile (256) with holes that move matches across those
edges, 8192 slots, iteration counts around the sixteen-hypotheses pass and the 32-hypotheses chunk of the count, ragged problems with all three statuses
in one call, recompute on and off with refits over 8, 64, 65 and 257 inliers, caller's and drawn samples, the degenerate samples of the CPU
census, NaN scores, ties between lane groups, passes and chunks (the atomic maximum), absent optional outputs, and two calls back to back on one stream.  Both
paths into the 9 x 9 Jacobi (a lane group per hypothesis, wave 0 of the refit) run in every OK problem with recompute."""
import numpy as np
import pytest

import two_view_scene as S
from plp import plp

pytestmark = pytest.mark.gpu
SENT = {np.dtype(np.uint8): 0xA5, np.dtype(np.int32): -77777, np.dtype(np.float64): -987.25, np.dtype(np.float32): np.float32(-321.5)}
OPTIONAL = ("inliers", "hyp_score")
PASS = 16   # kEssPass of csrc/essential_kernels.hip: hypotheses per workgroup of k_ess_hypotheses
CHUNK = 32  # kEssChunk: hypotheses per workgroup of k_ess_count


@pytest.fixture(scope="module")
def mt():
    return plp.matcher()


def sentinels(P, n_cap, iters):
    return {k: np.full((P,) + shape(n_cap, iters), SENT[np.dtype(dt)], dt) for k, (shape, dt, _) in plp.ESSENTIAL_OUTPUTS.items()}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def call_args(a, iters, recompute, use_seed):
    pos = (a["bearing_1"], a["bearing_2"], a["match"])
    kw = dict(iters=iters, recompute=recompute, counts_1=a["counts_1"], counts_2=a["counts_2"])
    kw.update(dict(seed=use_seed) if use_seed is not None else dict(samples=a["samples"]))
    return pos, kw


def enqueue_device(mt, a, iters, recompute, use_seed, skip_optional=False, stream=None):
    """plp_essential_ransac_device on sentinel-filled device outputs; returns the output tensors (nothing is synchronised)"""
    import torch
    P, n_cap = a["match"].shape
    d = lambda v: torch.from_numpy(np.ascontiguousarray(v).copy()).cuda()
    o = {k: d(v) for k, v in sentinels(P, n_cap, iters).items()}
    passed = {k: v for k, v in o.items() if not (skip_optional and k in OPTIONAL)}
    dev = {k: d(a[k]) for k in ("bearing_1", "bearing_2", "match", "counts_1", "counts_2", "samples")}
    mt.essential_ransac_device(P, n_cap, a["bearing_2"].shape[1], dev["bearing_1"], dev["bearing_2"], dev["match"], passed, iters=iters, recompute=recompute,
                               samples=None if use_seed is not None else dev["samples"], seed=use_seed or 0, counts_1=dev["counts_1"],
                               counts_2=dev["counts_2"], stream=stream)
    return o, dev


def check(mt, problems, recompute=True, use_seed=None, n_cap=None, host=True, skip_optional=False):
    import torch
    a = S.pack(problems, n_cap)
    P, n_cap = a["match"].shape
    iters = a["samples"].shape[1]
    pos, kw = call_args(a, iters, recompute, use_seed)
    want = plp.model_essential_ransac(*pos, out=sentinels(P, n_cap, iters), **kw)
    for p in range(P):                                            # the model itself leaves the slots above a count alone
        assert (want["inliers"][p, int(a["counts_1"][p]):] == SENT[np.dtype(np.uint8)]).all()
    o, _ = enqueue_device(mt, a, iters, recompute, use_seed, skip_optional)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in o.items()}
    for k in want:
        if skip_optional and k in OPTIONAL:
            assert (got[k] == SENT[got[k].dtype]).all(), ("an output that was not passed was written", k)
        else:
            assert same_bits(got[k], want[k]), ("device", k, got[k], want[k])
    if host:
        h = mt.essential_ransac(*pos, out=sentinels(P, n_cap, iters), **kw)
        for k in want:
            assert same_bits(h[k], want[k]), ("host entry", k)
    return want


# n = 7 / 8 / 9: the sample size; 63 / 64 / 65: the wave edge; 255 / 256 / 257: the compaction chunk and the LDS tile; 513: the third tile
@pytest.mark.parametrize("n", [7, 8, 9, 63, 64, 65, 255, 256, 257, 513])
def test_numbers_of_matches_around_every_edge(mt, n):
    model = S.MODELS[n % 3]
    dense = S.problem(100 + n, n, model, noise=1e-3 if n > 9 else 0.0, mismatch=0.0 if n <= 9 else 0.3)
    holes = S.problem(200 + n, n, model, n_slots=2 * n + 7, noise=1e-3 if n > 9 else 0.0)   # matches cross the wave and chunk edges at other slots
    for recompute in (True, False):
        w = check(mt, [dense, holes], recompute=recompute, host=recompute)
        assert w["num_matches"].tolist() == [n, n]
        assert (w["status"] == (plp.ESSENTIAL_TOO_FEW_MATCHES if n < 8 else plp.ESSENTIAL_OK)).all()


def test_8192_slots(mt):
    q = S.problem(31, 700, "equirectangular", n_slots=8192, noise=1e-3, mismatch=0.2, iters=17)
    w = check(mt, [q], host=False)
    assert w["status"][0] == plp.ESSENTIAL_OK and w["num_matches"][0] == 700


@pytest.mark.parametrize("iters", [1, PASS - 1, PASS, PASS + 1, CHUNK - 1, CHUNK, CHUNK + 1, 50, 100, 257])
def test_iteration_counts_around_the_pass_and_the_chunk(mt, iters):
    qs = [S.problem(300 + iters + p, 70 + p, S.MODELS[p], n_slots=90, noise=1e-3, mismatch=0.25, iters=iters) for p in range(3)]
    check(mt, qs, host=False)
    check(mt, qs, use_seed=77 + iters, recompute=False, host=False)               # drawn samples


def test_ragged_problems_reach_all_three_statuses_in_one_call(mt):
    qs = [S.problem(41, 120, "perspective", n_slots=150, noise=1e-3, mismatch=0.2), S.problem(42, 3, "fisheye"),
          S.problem(43, 40, "equirectangular", mismatch=1.0), S.problem(44, 300, "equirectangular", n_slots=333, noise=2e-3, mismatch=0.4),
          S.problem(45, 7, "perspective"), S.problem(46, 65, "fisheye", n_slots=129, noise=1e-3), S.nan_problem(), S.problem(47, 0, "fisheye", n_slots=5)]
    for q in qs:
        q["samples"], q["iters"] = q["samples"][:6], 6
    w = check(mt, qs)
    assert set(w["status"].tolist()) == {plp.ESSENTIAL_OK, plp.ESSENTIAL_TOO_FEW_MATCHES, plp.ESSENTIAL_INVALID}
    assert w["status"][6] == plp.ESSENTIAL_INVALID and np.isnan(w["hyp_score"][6]).all()
    check(mt, qs, use_seed=5, host=False)


@pytest.mark.parametrize("recompute", [False, True])
@pytest.mark.parametrize("n_in", [8, 64, 65, 257])
def test_refit_over_inlier_counts_around_every_edge(mt, recompute, n_in):
    """six gross mismatches among n_in exact matches and samples of exact matches only: the best hypothesis has exactly n_in inliers"""
    q = S.problem(500 + n_in, n_in + 6, S.MODELS[n_in % 3], n_slots=n_in + 20, iters=8)
    slots = np.flatnonzero(q["match"] >= 0)
    is_out = np.zeros(n_in + 6, bool)
    is_out[[1, 3, n_in // 2, n_in, n_in + 2, n_in + 5]] = True
    rng = np.random.default_rng(n_in)
    q["bearing_2"][q["match"][slots[is_out]]] = S.unit(q["bearing_2"][q["match"][slots[is_out]]] + S.unit(rng.standard_normal((6, 3))))
    good = np.flatnonzero(~is_out)
    for i in range(8):
        q["samples"][i] = rng.permutation(good)[:8]
    w = check(mt, [q], recompute=recompute)
    assert w["status"][0] == plp.ESSENTIAL_OK and w["num_inliers"][0] == n_in


def test_degenerate_samples(mt):
    q = S.degenerate_problem()
    w = check(mt, [q])
    h = w["hyp_score"][0]
    assert h[0] == 0 and h[1] == 0 and h[2] == 0 and h[3] == h[4] and np.isfinite(h).all() and w["best_iter"][0] >= 3, h


def test_ties_between_lane_groups_waves_and_passes(mt):
    """the same sample at several iterations: equal scores in two lane groups of a workgroup of k_ess_hypotheses and two lanes of one of
    k_ess_count (3, 5), in two workgroups of the former (3, 20) and in two of both (3, 37); the lowest iteration wins.  The other samples are made of mismatches, whose scores stay below."""
    q = S.problem(81, 90, "fisheye", n_slots=100, noise=2e-3, mismatch=0.0, iters=40)
    w0 = check(mt, [q], recompute=False, host=False)
    top = int(np.argmax(w0["hyp_score"][0]))
    for i in (3, 5, 20, 37):
        q["samples"][i] = q["samples"][top]
    if top not in (3, 5, 20, 37):
        q["samples"][top] = q["samples"][(top + 1) % 40 if (top + 1) % 40 not in (3, 5, 20, 37) else (top + 2) % 40]
    w = check(mt, [q], recompute=False)
    assert w["best_iter"][0] == 3 and len(set(w["hyp_score"][0][[3, 5, 20, 37]].tolist())) == 1
    assert w["hyp_score"][0].max() == w["hyp_score"][0][3]


def test_optional_outputs_absent(mt):
    qs = [S.problem(91, 80, "perspective", n_slots=100, noise=1e-3), S.problem(92, 5, "fisheye")]
    check(mt, qs, skip_optional=True, host=False)


def test_two_calls_back_to_back_on_one_stream(mt):
    """the second call reuses the context's buffers behind the first on the same stream, with nothing synchronised in between"""
    import torch
    a1 = S.pack([S.problem(95, 130, "equirectangular", n_slots=160, noise=1e-3, mismatch=0.2), S.problem(96, 20, "perspective")])
    a2 = S.pack([S.problem(97, 64, "fisheye", n_slots=70, noise=1e-3)])
    o1, k1 = enqueue_device(mt, a1, 24, True, None)
    o2, k2 = enqueue_device(mt, a2, 24, True, 9)
    torch.cuda.synchronize()
    for a, o, seed in ((a1, o1, None), (a2, o2, 9)):
        P, n_cap = a["match"].shape
        pos, kw = call_args(a, 24, True, seed)
        want = plp.model_essential_ransac(*pos, out=sentinels(P, n_cap, 24), **kw)
        for k in want:
            assert same_bits(o[k].cpu().numpy(), want[k]), k


def test_mirror_class_on_the_device(mt):
    q = S.problem(99, 60, "perspective", n_slots=70, noise=1e-3, mismatch=0.2)
    pairs = [(s, int(m)) for s, m in enumerate(q["match"]) if m >= 0]
    s = plp.essential_solver(q["bearing_1"], q["bearing_2"], pairs, mt=mt, samples=q["samples"])
    s.find_via_ransac(24)
    m = plp.essential_solver(q["bearing_1"], q["bearing_2"], pairs, samples=q["samples"])
    m.find_via_ransac(24)
    assert s.solution_is_valid() and m.solution_is_valid()
    assert same_bits(s.get_best_E_21(), m.get_best_E_21()) and same_bits(s.get_inlier_matches(), m.get_inlier_matches())
    assert s.get_best_score() == m.get_best_score() and len(s.get_inlier_matches()) == 60


def test_argument_checks_of_both_entries(mt):
    """a bad argument is refused before anything is written; P == 0 or n_cap == 0 writes nothing"""
    import torch
    a = S.pack([S.problem(1, 12, "perspective")])
    pos = (a["bearing_1"], a["bearing_2"], a["match"])
    out = sentinels(1, 12, 1)
    with pytest.raises(plp.PlpError) as e:
        mt.essential_ransac(*pos, iters=0, out=out)
    assert e.value.status == plp.PLP_ERR_INVALID_ARG and all((v == SENT[v.dtype]).all() for v in out.values())
    with pytest.raises(plp.PlpError) as e:
        mt.essential_ransac(np.zeros((1, 8193, 3)), np.zeros((1, 4, 3)), np.zeros((1, 8193), np.int32))
    assert e.value.status == plp.PLP_ERR_UNSUPPORTED
    d = lambda v: torch.from_numpy(np.ascontiguousarray(v).copy()).cuda()
    o = {k: d(v) for k, v in sentinels(1, 12, 24).items()}
    dev = [d(v) for v in pos]
    m_cap = a["bearing_2"].shape[1]
    with pytest.raises(plp.PlpError) as e:
        mt.essential_ransac_device(1, 12, m_cap, *dev, o, iters=0)
    assert e.value.status == plp.PLP_ERR_INVALID_ARG
    with pytest.raises(plp.PlpError) as e:
        mt.essential_ransac_device(1, 12, -1, *dev, o)
    assert e.value.status == plp.PLP_ERR_INVALID_ARG
    with pytest.raises(plp.PlpError) as e:
        mt.essential_ransac_device(1, 12, m_cap, dev[0], None, dev[2], o)
    assert e.value.status == plp.PLP_ERR_INVALID_ARG
    with pytest.raises(plp.PlpError) as e:
        mt.essential_ransac_device(1, 12, m_cap, *dev, {k: v for k, v in o.items() if k != "score"})
    assert e.value.status == plp.PLP_ERR_INVALID_ARG
    mt.essential_ransac_device(0, 12, m_cap, *dev, o)                              # nothing to do
    mt.essential_ransac_device(1, 0, 0, None, None, None, {})
    torch.cuda.synchronize()
    for k, v in o.items():
        assert (v.cpu().numpy() == SENT[np.dtype(plp.ESSENTIAL_OUTPUTS[k][1])]).all(), k


def test_initializer_step_runs_both_callers_without_the_host(mt):
    """initializer_step.essential is find_via_ransac(100, true), robust_inliers is find_via_ransac(50, false) with zero matches where the
    solution is not valid, both on tensors that stay on the device"""
    import importlib

    import torch
    step_mod = importlib.import_module(plp.__name__ + ".initializer_step")
    qs = [S.problem(61, 150, "fisheye", n_slots=170, noise=1e-3, mismatch=0.3), S.problem(62, 40, "equirectangular", mismatch=1.0),
          S.problem(63, 5, "perspective", n_slots=9)]
    a = S.pack(qs)
    d = lambda v: torch.from_numpy(np.ascontiguousarray(v).copy()).cuda()
    step = step_mod.initializer_step(plp, mt=mt)
    args = [d(a[k]) for k in ("bearing_1", "bearing_2", "match")]
    kw = dict(counts_1=d(a["counts_1"]), counts_2=d(a["counts_2"]), seed=13)
    e = step.essential(*args, **kw)
    r = step.robust_inliers(*args, **kw)
    torch.cuda.synchronize()
    pos = (a["bearing_1"], a["bearing_2"], a["match"])
    hk = dict(counts_1=a["counts_1"], counts_2=a["counts_2"], seed=13, outputs=("inliers",))
    we = plp.model_essential_ransac(*pos, iters=100, recompute=True, **hk)
    wr = plp.model_essential_ransac(*pos, iters=50, recompute=False, **hk)
    for k in we:
        assert same_bits(e[k].cpu().numpy(), we[k]), k
    assert same_bits(r["inliers"].cpu().numpy(), wr["inliers"]) and same_bits(r["num_inlier_matches"].cpu().numpy(), wr["num_inliers"])
    assert we["status"].tolist() == [plp.ESSENTIAL_OK, plp.ESSENTIAL_INVALID, plp.ESSENTIAL_TOO_FEW_MATCHES]
    assert wr["num_inliers"][0] > 8 and wr["num_inliers"][1] == 0 and not wr["inliers"][1].any()
