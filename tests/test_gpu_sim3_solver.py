"""solve::sim3_solver on the device (plp_sim3_ransac_device / _host, csrc/sim3_kernels.hip) against the CPU build of the same header
(plp.model_sim3_ransac, which tests/test_sim3_solver_cpu.py holds bit for bit to the restatement tests/sim3_solver_ref.py; DESIGN.md section 5,
D13): every output bit for bit on sentinel-filled arrays, at the smallest shapes at which the kernels can go wrong -- numbers of common points
around the wave (64), the workgroup and the LDS tile (256) with holes that move ranks across those edges, 8192 slots, iteration counts around
the 256-hypothesis chunk, ragged problems with all three statuses in one call, every camera, both scale modes, caller's and drawn samples,
ties between waves and between chunks, and two calls back to back on one stream."""
import numpy as np
import pytest

import sim3_solver_scene as S
from plp import plp

pytestmark = pytest.mark.gpu
SENT = {np.dtype(np.uint8): 0xA5, np.dtype(np.int32): -77777, np.dtype(np.float32): np.float32(-123.5), np.dtype(np.float64): -987.25}
OPTIONAL = ("inliers", "hyp_inliers")


@pytest.fixture(scope="module")
def mt():
    return plp.matcher()


def sentinels(P, n_cap, iters):
    return {k: np.full((P,) + shape(n_cap, iters), SENT[np.dtype(dt)], dt) for k, (shape, dt, _) in plp.SIM3_OUTPUTS.items()}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def call_args(name, a, fix, iters, min_inl, use_seed):
    cam = plp.camera_model(S.CAMERAS[name])
    pos = (cam, a["valid"], a["pos_w_1"], a["pos_w_2"], a["octave_1"], a["octave_2"], a["pose_1"], a["pose_2"], S.SIGMA_SQ, S.SIGMA_SQ)
    kw = dict(iters=iters, fix_scale=fix, min_num_inliers=min_inl, counts=a["counts"])
    kw.update(dict(seed=use_seed) if use_seed is not None else dict(samples=a["samples"]))
    return pos, kw


def enqueue_device(mt, name, a, fix, iters, min_inl, use_seed, skip_optional=False, stream=None):
    """plp_sim3_ransac_device on sentinel-filled device outputs; returns the output tensors (nothing is synchronised)"""
    import torch
    P, n_cap = a["valid"].shape
    d = lambda v: torch.from_numpy(np.ascontiguousarray(v).copy()).cuda()
    o = {k: d(v) for k, v in sentinels(P, n_cap, iters).items()}
    passed = {k: v for k, v in o.items() if not (skip_optional and k in OPTIONAL)}
    dev = {k: d(a[k]) for k in ("valid", "pos_w_1", "pos_w_2", "octave_1", "octave_2", "pose_1", "pose_2", "counts", "samples")}
    mt.sim3_ransac_device(plp.camera_model(S.CAMERAS[name]), P, n_cap, dev["valid"], dev["pos_w_1"], dev["pos_w_2"], dev["octave_1"], dev["octave_2"],
                          dev["pose_1"], dev["pose_2"], S.SIGMA_SQ, S.SIGMA_SQ, passed, iters=iters, fix_scale=fix, min_num_inliers=min_inl,
                          samples=None if use_seed is not None else dev["samples"], seed=use_seed or 0, counts=dev["counts"], stream=stream)
    return o, dev


def check(mt, name, problems, fix=False, min_inl=20, use_seed=None, n_cap=None, host=True, skip_optional=False):
    import torch
    a = S.pack(problems, n_cap)
    P, n_cap = a["valid"].shape
    iters = problems[0]["iters"]
    pos, kw = call_args(name, a, fix, iters, min_inl, use_seed)
    want = plp.model_sim3_ransac(*pos, out=sentinels(P, n_cap, iters), **kw)
    for p, q in enumerate(problems):                              # the model itself leaves the slots above a count alone
        assert (want["inliers"][p, len(q["valid"]):] == SENT[np.dtype(np.uint8)]).all()
    o, _ = enqueue_device(mt, name, a, fix, iters, min_inl, use_seed, skip_optional)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in o.items()}
    for k in want:
        if skip_optional and k in OPTIONAL:
            assert (got[k] == SENT[got[k].dtype]).all(), ("an output that was not passed was written", k)
        else:
            assert same_bits(got[k], want[k]), ("device", name, k, got[k], want[k])
    if host:
        h = mt.sim3_ransac(*pos, out=sentinels(P, n_cap, iters), **kw)
        for k in want:
            assert same_bits(h[k], want[k]), ("host entry", name, k)
    return want


# n = 64 / 65: the wave edge; 256 / 257: the workgroup and the LDS tile; 513: the third tile; 19 / 20: min_num_inliers
@pytest.mark.parametrize("n", [2, 3, 19, 20, 63, 64, 65, 256, 257, 513])
def test_numbers_of_common_points_around_every_edge(mt, n):
    q = S.problem(100 + n, n, n_slots=n + n // 2 + 5, outliers=0.3, iters=200)      # the holes move ranks across wave and workgroup boundaries
    want = check(mt, "perspective", [q])
    st = int(want["status"][0])
    # 20 common points pass :130 and run the loop; with 30 % outliers they cannot reach 20 inliers (:177)
    assert st == (plp.SIM3_TOO_FEW_POINTS if n < 20 else plp.SIM3_TOO_FEW_INLIERS if n == 20 else plp.SIM3_OK), (n, st)
    assert int(want["num_common"][0]) == n
    if n >= 20:
        assert int(want["num_inliers"][0]) >= 0.5 * n and (int(want["best_iter"][0]) >= 0) == (n > 20)


def test_three_points_are_enough_when_the_caller_asks_for_no_more(mt):
    for n in (2, 3):
        q = S.problem(7, n, n_slots=6, outliers=0.0, iters=64)
        want = check(mt, "perspective", [q], min_inl=0)
        assert int(want["status"][0]) == (plp.SIM3_OK if n == 3 else plp.SIM3_TOO_FEW_POINTS)


def test_8192_slots_with_few_common_points(mt):
    q = S.problem(11, 40, n_slots=8192, outliers=0.3, iters=200)
    want = check(mt, "perspective", [q], host=False)
    assert int(want["status"][0]) == plp.SIM3_OK and int(want["num_common"][0]) == 40


@pytest.mark.parametrize("iters", [1, 64, 200, 256, 257, 600])
def test_iteration_counts_around_the_chunk_of_256(mt, iters):
    q = S.problem(200 + iters, 65, n_slots=90, outliers=0.3, iters=iters)
    check(mt, "fisheye", [q], min_inl=20 if iters > 1 else 0)


@pytest.mark.parametrize("name", sorted(S.CAMERAS))
@pytest.mark.parametrize("fix", [False, True])
def test_seven_ragged_problems_with_all_three_statuses(mt, name, fix):
    probs = [S.problem(300, 70, 100, 0.4, fix), S.problem(301, 2, 9, 0.0, fix), S.problem(302, 30, 30, 0.4, fix, all_outliers=True),
             S.problem(303, 257, 300, 0.5, fix, behind_own=2), S.problem(304, 19, 40, 0.2, fix), S.problem(305, 130, 131, 0.3, fix),
             S.problem(306, 24, 64, 0.3, fix)]
    want = check(mt, name, probs)
    assert set(want["status"].tolist()) == {plp.SIM3_OK, plp.SIM3_TOO_FEW_POINTS, plp.SIM3_TOO_FEW_INLIERS}, want["status"]
    bad = want["status"] != plp.SIM3_OK
    assert (want["best_iter"][bad] == -1).all() and not want["rot_12"][bad].any() and not want["scale_12"][bad].any()
    for p in np.flatnonzero(bad):
        assert not want["inliers"][p, :len(probs[p]["valid"])].any()


@pytest.mark.parametrize("name", sorted(S.CAMERAS))
def test_samples_drawn_on_the_device_are_the_host_models(mt, name):
    probs = [S.problem(400, 70, 100, 0.4), S.problem(401, 7, 12, 0.0), S.problem(402, 300, 300, 0.5)]
    want = check(mt, name, probs, use_seed=0x1234567890ABCDEF, min_inl=5)
    assert (want["status"] == plp.SIM3_OK).all()


def test_bad_samples_give_hypotheses_without_inliers(mt):
    q = S.problem(500, 60, 80, 0.3, iters=64)
    q["samples"][3] = (5, 5, 9)            # a repeated index
    q["samples"][10] = (0, 60, 1)          # one past the last common point
    q["samples"][11] = (-1, 2, 3)
    want = check(mt, "perspective", [q])
    assert not want["hyp_inliers"][0, [3, 10, 11]].any() and int(want["status"][0]) == plp.SIM3_OK


def test_a_tie_goes_to_the_lowest_iteration_across_waves_and_chunks(mt):
    q = S.problem(600, 80, 100, 0.3, iters=600)
    good = np.flatnonzero(~q["is_outlier"])[:3]
    q["samples"][:] = (1, 1, 2)                                   # every other hypothesis: no inliers
    for it in (130, 70, 300, 520):                                # waves 2 and 1 of the first chunk, the second and the third chunk
        q["samples"][it] = good
    want = check(mt, "perspective", [q])
    h = want["hyp_inliers"][0]
    assert int(want["best_iter"][0]) == 70 and h[70] == h[130] == h[300] == h[520] == want["num_inliers"][0] >= 20
    assert np.count_nonzero(h) == 4


def test_optional_outputs_that_are_not_passed_are_not_written(mt):
    check(mt, "perspective", [S.problem(700, 50, 70, 0.3, iters=64)], skip_optional=True, host=False)


def test_two_calls_back_to_back_on_one_stream(mt):
    """the second call reuses (and regrows) the context buffers of the first while the first may still run: the stream orders them"""
    import torch
    a1 = S.pack([S.problem(800, 40, 60, 0.3, iters=64)])
    a2 = S.pack([S.problem(801 + i, 100 + 30 * i, 260, 0.4, iters=300) for i in range(5)])
    o1, keep1 = enqueue_device(mt, "perspective", a1, False, 64, 20, None)
    o2, keep2 = enqueue_device(mt, "equirectangular", a2, True, 300, 20, None)
    torch.cuda.synchronize()
    for name, a, o, fix, iters in (("perspective", a1, o1, False, 64), ("equirectangular", a2, o2, True, 300)):
        pos, kw = call_args(name, a, fix, iters, 20, None)
        P, n_cap = a["valid"].shape
        want = plp.model_sim3_ransac(*pos, out=sentinels(P, n_cap, iters), **kw)
        for k in want:
            assert same_bits(o[k].cpu().numpy(), want[k]), (name, k)


def test_the_mirror_class_runs_the_device_entry(mt):
    q = S.problem(900, 60, 80, 0.3)
    cam = plp.camera_model(S.CAMERAS["perspective"])
    args = (cam, q["valid"], q["pos_w_1"], q["pos_w_2"], q["octave_1"], q["octave_2"], q["pose_1"], q["pose_2"], S.SIGMA_SQ, S.SIGMA_SQ)
    dev, cpu = plp.sim3_solver(*args, mt=mt, samples=q["samples"]), plp.sim3_solver(*args, samples=q["samples"])
    for s in (dev, cpu):
        s.find_via_ransac(200)
    assert dev.solution_is_valid() and cpu.solution_is_valid()
    assert same_bits(dev.get_best_rotation_12(), cpu.get_best_rotation_12()) and same_bits(dev.get_best_translation_12(), cpu.get_best_translation_12())
    assert dev.get_best_scale_12() == cpu.get_best_scale_12() and np.array_equal(dev.get_inliers(), cpu.get_inliers())
