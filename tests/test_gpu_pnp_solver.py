"""solve::pnp_solver on the device (plp_pnp_ransac_device / _host, csrc/pnp_kernels.hip) against the CPU build of the same header
(plp.model_pnp_ransac, which tests/test_pnp_solver_cpu.py holds bit for bit to the restatement tests/pnp_solver_ref.py; DESIGN.md section 5,
D14): every output bit for bit on sentinel-filled arrays, at the smallest shapes at which the kernels can go wrong -- numbers of matches
around min_num_inliers, the wave (64), the workgroup and the LDS tile (256) with holes that move ranks across those edges, 8192 slots,
iteration counts around the sixteen-hypotheses pass, ragged problems with all three statuses in one call, recompute on and off with refits
over 4, 64, 65 and 257 inliers, caller's and drawn samples, the degenerate samples of the CPU census, ties between lane groups, waves and
passes, absent optional outputs, and two calls back to back on one stream.  Both paths into the 12 x 12 Jacobi (a lane group per hypothesis,
wave 0 of the refit) run in every OK problem with recompute."""
import numpy as np
import pytest

import pnp_solver_scene as S
from plp import plp

pytestmark = pytest.mark.gpu
SENT = {np.dtype(np.uint8): 0xA5, np.dtype(np.int32): -77777, np.dtype(np.float64): -987.25}
OPTIONAL = ("inliers", "hyp_inliers")
PASS = 16   # kPnpPass of csrc/pnp_kernels.hip: hypotheses per workgroup pass


@pytest.fixture(scope="module")
def mt():
    return plp.matcher()


def sentinels(P, n_cap, iters):
    return {k: np.full((P,) + shape(n_cap, iters), SENT[np.dtype(dt)], dt) for k, (shape, dt, _) in plp.PNP_OUTPUTS.items()}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def call_args(a, iters, min_inl, recompute, use_seed):
    pos = (a["valid"], a["bearing"], a["pos_w"], a["octave"], S.SCALE_FACTORS)
    kw = dict(iters=iters, min_num_inliers=min_inl, recompute=recompute, counts=a["counts"])
    kw.update(dict(seed=use_seed) if use_seed is not None else dict(samples=a["samples"]))
    return pos, kw


def enqueue_device(mt, a, iters, min_inl, recompute, use_seed, skip_optional=False, stream=None):
    """plp_pnp_ransac_device on sentinel-filled device outputs; returns the output tensors (nothing is synchronised)"""
    import torch
    P, n_cap = a["valid"].shape
    d = lambda v: torch.from_numpy(np.ascontiguousarray(v).copy()).cuda()
    o = {k: d(v) for k, v in sentinels(P, n_cap, iters).items()}
    passed = {k: v for k, v in o.items() if not (skip_optional and k in OPTIONAL)}
    dev = {k: d(a[k]) for k in ("valid", "bearing", "pos_w", "octave", "counts", "samples")}
    mt.pnp_ransac_device(P, n_cap, dev["valid"], dev["bearing"], dev["pos_w"], dev["octave"], S.SCALE_FACTORS, passed, iters=iters, min_num_inliers=min_inl,
                         recompute=recompute, samples=None if use_seed is not None else dev["samples"], seed=use_seed or 0, counts=dev["counts"],
                         stream=stream)
    return o, dev


def check(mt, problems, min_inl=10, recompute=True, use_seed=None, n_cap=None, host=True, skip_optional=False, arrays=None):
    import torch
    a = S.pack(problems, n_cap) if arrays is None else arrays
    P, n_cap = a["valid"].shape
    iters = a["samples"].shape[1]
    pos, kw = call_args(a, iters, min_inl, recompute, use_seed)
    want = plp.model_pnp_ransac(*pos, out=sentinels(P, n_cap, iters), **kw)
    for p in range(P):                                            # the model itself leaves the slots above a count alone
        assert (want["inliers"][p, int(a["counts"][p]):] == SENT[np.dtype(np.uint8)]).all()
    o, _ = enqueue_device(mt, a, iters, min_inl, recompute, use_seed, skip_optional)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in o.items()}
    for k in want:
        if skip_optional and k in OPTIONAL:
            assert (got[k] == SENT[got[k].dtype]).all(), ("an output that was not passed was written", k)
        else:
            assert same_bits(got[k], want[k]), ("device", k, got[k], want[k])
    if host:
        h = mt.pnp_ransac(*pos, out=sentinels(P, n_cap, iters), **kw)
        for k in want:
            assert same_bits(h[k], want[k]), ("host entry", k)
    return want


# n = 3 / 4: the sample size; 10 / 11: min_num_inliers (strict); 64 / 65: the wave edge; 256 / 257: the workgroup and the LDS tile; 513: the third tile
@pytest.mark.parametrize("n", [3, 4, 10, 11, 63, 64, 65, 256, 257, 513])
def test_numbers_of_matches_around_every_edge(mt, n):
    model = S.MODELS[n % 3]
    dense = S.problem(100 + n, n, model, iters=30, outliers=0.0 if n <= 11 else 0.3)
    holes = S.problem(200 + n, n, model, n_slots=2 * n + 7, iters=30)             # ranks cross the wave and workgroup edges at other slots
    w = check(mt, [dense, holes])
    assert w["num_matches"].tolist() == [n, n]
    if n < 10:
        assert (w["status"] == plp.PNP_TOO_FEW_MATCHES).all()
    elif n == 10:
        assert w["status"][0] == plp.PNP_TOO_FEW_INLIERS and w["num_inliers"][0] == 10    # all ten are inliers, and ten is not more than ten
    elif n == 11:
        assert w["status"][0] == plp.PNP_OK and w["num_inliers"][0] == 11
    else:
        assert (w["status"] == plp.PNP_OK).all()


def test_8192_slots(mt):
    q = S.problem(31, 700, "equirectangular", n_slots=8192, iters=17)
    w = check(mt, [q], host=False)
    assert w["status"][0] == plp.PNP_OK and w["num_matches"][0] == 700


@pytest.mark.parametrize("iters", [1, PASS - 1, PASS, PASS + 1, 30, 2 * PASS + 1])
def test_iteration_counts_around_the_pass(mt, iters):
    qs = [S.problem(300 + iters + p, 70 + p, S.MODELS[p], n_slots=90, iters=iters) for p in range(3)]
    check(mt, qs, host=False)
    check(mt, qs, use_seed=77 + iters, host=False)                                # drawn samples


def test_ragged_problems_reach_all_three_statuses_in_one_call(mt):
    qs = [S.problem(41, 120, "perspective", n_slots=150), S.problem(42, 3, "fisheye"), S.problem(43, 40, "equirectangular", all_outliers=True),
          S.problem(44, 300, "equirectangular", n_slots=333), S.problem(45, 9, "perspective"), S.problem(46, 65, "fisheye", n_slots=129)]
    w = check(mt, qs)
    assert set(w["status"].tolist()) == {plp.PNP_OK, plp.PNP_TOO_FEW_MATCHES, plp.PNP_TOO_FEW_INLIERS}
    check(mt, qs, use_seed=5, host=False)


@pytest.mark.parametrize("recompute", [False, True])
@pytest.mark.parametrize("n_in", [4, 64, 65, 257])
def test_refit_over_inlier_counts_around_every_edge(mt, recompute, n_in):
    """six outliers among n_in exact matches and samples of exact matches only: the best hypothesis has exactly n_in inliers (the seeds are
    the first from 500 on that give one; 4-point EPnP does not recover every exact sample)"""
    seed = 501 if n_in == 4 else 500
    q = S.problem(seed, n_in + 6, S.MODELS[n_in % 3], n_slots=n_in + 20, outliers=0.0, iters=8)
    is_out = np.zeros(n_in + 6, bool)
    is_out[[1, 3, n_in // 2, n_in, n_in + 2, n_in + 5]] = True
    slots = np.flatnonzero(q["valid"])
    rng = np.random.default_rng(seed)
    q["bearing"][slots[is_out]] = S.directions(rng, 6, np.pi)
    good = np.flatnonzero(~is_out)
    for i in range(8):
        q["samples"][i] = rng.permutation(good)[:4]
    w = check(mt, [q], min_inl=3, recompute=recompute)
    assert w["status"][0] == plp.PNP_OK and w["num_inliers"][0] == n_in


def test_degenerate_samples(mt):
    q = S.degenerate_problem()
    w = check(mt, [q], min_inl=5)
    h = w["hyp_inliers"][0]
    assert h[0] == 0 and h[1] == 0 and h[2] == 0 and h[6] == 0, h


def test_ties_between_lane_groups_waves_and_passes(mt):
    """the same sample at several iterations: equal counts in two lane groups of a wave (3, 5), in two waves (3, 20) and in two passes (3, 37);
    the lowest iteration wins"""
    q = S.problem(81, 90, "fisheye", n_slots=100, outliers=0.2, iters=40)
    good = np.flatnonzero(~q["is_outlier"])
    bad = np.flatnonzero(q["is_outlier"])
    for i in range(40):
        q["samples"][i] = [bad[i % len(bad)], good[i % len(good)], bad[(i + 1) % len(bad)], good[(i + 3) % len(good)]]
    for i in (3, 5, 20, 37):
        q["samples"][i] = good[[2, 7, 12, 17]]                                       # exact matches whose 4-point fit recovers the pose
    w = check(mt, [q])
    assert w["best_iter"][0] == 3 and len(set(w["hyp_inliers"][0][[3, 5, 20, 37]].tolist())) == 1


def test_optional_outputs_absent(mt):
    qs = [S.problem(91, 80, "perspective", n_slots=100), S.problem(92, 5, "fisheye")]
    check(mt, qs, skip_optional=True, host=False)


def test_two_calls_back_to_back_on_one_stream(mt):
    """the second call reuses the context's buffers behind the first on the same stream, with nothing synchronised in between"""
    import torch
    a1 = S.pack([S.problem(95, 130, "equirectangular", n_slots=160), S.problem(96, 20, "perspective")])
    a2 = S.pack([S.problem(97, 64, "fisheye", n_slots=70)])
    o1, k1 = enqueue_device(mt, a1, 30, 10, True, None)
    o2, k2 = enqueue_device(mt, a2, 30, 10, True, 9)
    torch.cuda.synchronize()
    for a, o, seed in ((a1, o1, None), (a2, o2, 9)):
        P, n_cap = a["valid"].shape
        pos, kw = call_args(a, 30, 10, True, seed)
        want = plp.model_pnp_ransac(*pos, out=sentinels(P, n_cap, 30), **kw)
        for k in want:
            assert same_bits(o[k].cpu().numpy(), want[k]), k


def test_mirror_class_on_the_device(mt):
    q = S.problem(99, 60, "perspective")
    s = plp.pnp_solver(q["bearing"], q["octave"], q["pos_w"], S.SCALE_FACTORS, mt=mt, samples=q["samples"])
    s.find_via_ransac(30)
    m = plp.pnp_solver(q["bearing"], q["octave"], q["pos_w"], S.SCALE_FACTORS, samples=q["samples"])
    m.find_via_ransac(30)
    assert s.solution_is_valid() and m.solution_is_valid()
    assert same_bits(s.get_best_cam_pose(), m.get_best_cam_pose()) and same_bits(s.get_inlier_flags(), m.get_inlier_flags())


def test_argument_checks_of_both_entries(mt):
    """a bad argument is refused before anything is written; P == 0 or n_cap == 0 writes nothing"""
    import torch
    a = S.pack([S.problem(1, 12, "perspective")])
    pos = (a["valid"], a["bearing"], a["pos_w"], a["octave"])
    for kw, status in ((dict(iters=0), plp.PLP_ERR_INVALID_ARG), (dict(min_num_inliers=-1), plp.PLP_ERR_INVALID_ARG)):
        out = sentinels(1, 12, max(kw.get("iters", 30), 1))
        with pytest.raises(plp.PlpError) as e:
            mt.pnp_ransac(*pos, S.SCALE_FACTORS, out=out, **kw)
        assert e.value.status == status and all((v == SENT[v.dtype]).all() for v in out.values())
    for sf in (S.SCALE_FACTORS[:0], np.ones(17, np.float32)):
        with pytest.raises(plp.PlpError) as e:
            mt.pnp_ransac(*pos, sf)
        assert e.value.status == plp.PLP_ERR_INVALID_ARG
    with pytest.raises(plp.PlpError) as e:
        mt.pnp_ransac(np.zeros((1, 8193), np.uint8), np.zeros((1, 8193, 3)), np.zeros((1, 8193, 3)), np.zeros((1, 8193), np.int32), S.SCALE_FACTORS)
    assert e.value.status == plp.PLP_ERR_UNSUPPORTED
    d = lambda v: torch.from_numpy(np.ascontiguousarray(v).copy()).cuda()
    o = {k: d(v) for k, v in sentinels(1, 12, 30).items()}
    dev = [d(v) for v in pos]
    with pytest.raises(plp.PlpError) as e:
        mt.pnp_ransac_device(1, 12, *dev, S.SCALE_FACTORS, o, iters=0)
    assert e.value.status == plp.PLP_ERR_INVALID_ARG
    with pytest.raises(plp.PlpError) as e:
        mt.pnp_ransac_device(1, 12, dev[0], None, dev[2], dev[3], S.SCALE_FACTORS, o)
    assert e.value.status == plp.PLP_ERR_INVALID_ARG
    with pytest.raises(plp.PlpError) as e:
        mt.pnp_ransac_device(1, 12, *dev, S.SCALE_FACTORS, {k: v for k, v in o.items() if k != "status"})
    assert e.value.status == plp.PLP_ERR_INVALID_ARG
    mt.pnp_ransac_device(0, 12, *dev, S.SCALE_FACTORS, o)                          # nothing to do
    mt.pnp_ransac_device(1, 0, None, None, None, None, S.SCALE_FACTORS, {})
    torch.cuda.synchronize()
    for k, v in o.items():
        assert (v.cpu().numpy() == SENT[np.dtype(plp.PNP_OUTPUTS[k][1])]).all(), k
