"""The homography and the fundamental RANSAC of initialize::perspective on the device (plp_perspective_ransac_device / _host,
csrc/perspective_init_kernels.hip) against the CPU build of the same header (plp.model_perspective_ransac, which tests/test_perspective_init_cpu.py
holds bit for bit to the restatement tests/perspective_init_ref.py): every output bit for bit on sentinel-filled arrays, at
the smallest shapes at which the kernels can go wrong -- numbers of matches around the sample size (8), the wave (64), the compaction chunk and the
LDS tile (256) with holes that move matches across those edges, frames whose key-point counts differ from their match counts around the 256
key points of a normalisation tile, 8192 slots, iteration counts around the sixteen-hypotheses pass and the 32-hypotheses chunk of the count, ragged
problems with every status of both solvers and all three choices in one call, a given homography mixed with RANSAC problems, recompute on and off
with refits over 8, 64, 65 and 257 inliers, caller's and drawn samples, degenerate samples, NaN and constant frames, ties between lane groups, passes
and chunks, absent optional outputs, and two calls back to back on one stream."""
import numpy as np
import pytest

import perspective_init_scene as S
from plp import plp

pytestmark = pytest.mark.gpu
SENT = {np.dtype(np.uint8): 0xA5, np.dtype(np.int32): -77777, np.dtype(np.float64): -987.25, np.dtype(np.float32): np.float32(-321.5)}
OPTIONAL = tuple(k for k, v in plp.PERSPECTIVE_RANSAC_OUTPUTS.items() if v[2])
PASS = 16   # kPerspPass of csrc/perspective_init_kernels.hip: hypotheses per workgroup of k_persp_hypotheses
CHUNK = 32  # kPerspChunk: hypotheses per workgroup of k_persp_count
OK, FEW, INVALID = plp.PERSPECTIVE_OK, plp.PERSPECTIVE_TOO_FEW_MATCHES, plp.PERSPECTIVE_INVALID


@pytest.fixture(scope="module")
def mt():
    return plp.matcher()


def sentinels(P, n_cap, iters):
    return {k: np.full((P,) + shape(n_cap, iters), SENT[np.dtype(dt)], dt) for k, (shape, dt, _) in plp.PERSPECTIVE_RANSAC_OUTPUTS.items()}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def to_device(v):
    import torch
    v = np.ascontiguousarray(v)
    return torch.from_numpy(v.view(np.uint8).copy() if v.dtype == plp.KP_DTYPE else v.copy()).cuda()


def enqueue_device(mt, a, recompute, seed, skip_optional=False, stream=None):
    """plp_perspective_ransac_device on sentinel-filled device outputs; returns the output tensors (nothing is synchronised)"""
    P, n_cap = a["match"].shape
    iters = a["samples_h"].shape[1]
    o = {k: to_device(v) for k, v in sentinels(P, n_cap, iters).items()}
    passed = {k: v for k, v in o.items() if not (skip_optional and k in OPTIONAL)}
    dev = {k: to_device(v) for k, v in a.items()}
    mt.perspective_ransac_device(P, n_cap, a["undist_2"].shape[1], dev["undist_1"], dev["undist_2"], dev["match"], passed, iters=iters, recompute=recompute,
                                 samples_h=None if seed is not None else dev["samples_h"], samples_f=None if seed is not None else dev["samples_f"],
                                 seed=seed or 0, counts_1=dev["counts_1"], counts_2=dev["counts_2"], given_H_21=dev.get("given_H_21"),
                                 given_H_num_inliers=dev.get("given_H_num_inliers"), stream=stream)
    return o, dev


def check(mt, problems, recompute=True, seed=None, n_cap=None, host=True, skip_optional=False, given=None):
    import torch
    a = S.pack(problems, n_cap, given=given)
    P, n_cap = a["match"].shape
    iters = a["samples_h"].shape[1]
    pos, kw = S.call_kwargs(a, recompute, seed)
    want = plp.model_perspective_ransac(*pos, out=sentinels(P, n_cap, iters), **kw)
    for p in range(P):                                            # the model itself leaves the slots above a count alone
        assert (want["inliers"][p, int(a["counts_1"][p]):] == SENT[np.dtype(np.uint8)]).all()
    o, _ = enqueue_device(mt, a, recompute, seed, skip_optional)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in o.items()}
    for k in want:
        if skip_optional and k in OPTIONAL:
            assert (got[k] == SENT[got[k].dtype]).all(), ("an output that was not passed was written", k)
        else:
            assert same_bits(got[k], want[k]), ("device", k, got[k], want[k])
    if host:
        h = mt.perspective_ransac(*pos, out=sentinels(P, n_cap, iters), **kw)
        for k in want:
            assert same_bits(h[k], want[k]), ("host entry", k)
    return want


# n = 7 / 8 / 9: the sample size; 63 / 64 / 65: the wave edge; 255 / 256 / 257: the compaction chunk and the LDS tiles; 513: the third tile
@pytest.mark.parametrize("n", [7, 8, 9, 63, 64, 65, 255, 256, 257, 513])
def test_numbers_of_matches_around_every_edge(mt, n):
    model = ("perspective", "fisheye")[n % 2]
    dense = S.problem(100 + n, n, model, noise=1e-3 if n > 9 else 0.0, mismatch=0.0 if n <= 9 else 0.3, iters=8)
    holes = S.problem(200 + n, n, model, n_slots=2 * n + 7, noise=1e-3 if n > 9 else 0.0, iters=8)   # matches cross the wave and tile edges at other slots
    for recompute in (True, False):
        w = check(mt, [dense, holes], recompute=recompute, host=recompute)
        assert w["num_matches"].tolist() == [n, n]
        assert (w["status_f"] == (FEW if n < 8 else OK)).all() and ((w["status_h"] == FEW) == (n < 8)).all()


@pytest.mark.parametrize("n1,n2", [(250, 255), (251, 256), (252, 257), (255, 300), (256, 512), (257, 513), (40, 600)])
def test_key_point_counts_around_the_normalisation_tile(mt, n1, n2):
    """frames of n1 and n2 key points with 40 matches among them: the four coordinate chains end at other tiles than the matches and than each other"""
    q = S.problem(700 + n1, 40, "perspective", n_slots=max(n1, 40), noise=1e-3, mismatch=0.1, iters=6)
    rng = np.random.default_rng(n1 * 1000 + n2)
    extra = np.zeros(max(n2 - len(q["undist_2"]), 0), plp.KP_DTYPE)
    extra["x"], extra["y"] = rng.uniform(0, 640, len(extra)), rng.uniform(0, 480, len(extra))
    q["undist_2"] = np.concatenate([q["undist_2"], extra.astype(plp.KP_DTYPE)])
    w = check(mt, [q], host=False)
    assert w["num_matches"][0] == 40 and w["status_f"][0] == OK and len(q["undist_1"]) == n1 and len(q["undist_2"]) == n2


def test_8192_slots(mt):
    q = S.problem(31, 700, "perspective", n_slots=8192, noise=1e-3, mismatch=0.2, iters=17)
    w = check(mt, [q], host=False)
    assert w["status_f"][0] == OK and w["num_matches"][0] == 700


@pytest.mark.parametrize("iters", [1, PASS - 1, PASS, PASS + 1, CHUNK - 1, CHUNK, CHUNK + 1, 100])
def test_iteration_counts_around_the_pass_and_the_chunk(mt, iters):
    qs = [S.problem(300 + iters + p, 70 + p, ("perspective", "fisheye")[p % 2], n_slots=90, noise=1e-3, mismatch=0.25, iters=iters,
                    kind=("cloud", "planar", "cloud")[p]) for p in range(3)]
    check(mt, qs, host=False)
    check(mt, qs, seed=77 + iters, recompute=False, host=False)               # drawn samples


def ragged():
    qs = [S.problem(41, 120, "perspective", n_slots=150, noise=5e-4, mismatch=0.05, kind="planar"), S.problem(42, 3, "fisheye"),
          S.problem(43, 40, "perspective", mismatch=1.0), S.problem(44, 300, "fisheye", n_slots=333, noise=2e-3, mismatch=0.4),
          S.problem(45, 7, "perspective"), S.problem(46, 65, "fisheye", n_slots=129, noise=1e-3), S.nan_problem(), S.problem(47, 0, "fisheye", n_slots=5),
          S.constant_frame_problem(), S.problem(48, 90, "perspective", noise=0.0)]
    for q in qs:
        q["samples_h"], q["samples_f"], q["iters"] = q["samples_h"][:6], q["samples_f"][:6], 6
    return qs


def test_ragged_problems_reach_every_status_and_choice_in_one_call(mt):
    qs = ragged()
    w = check(mt, qs)
    assert set(w["status_h"].tolist()) == set(w["status_f"].tolist()) == {OK, FEW, INVALID}
    assert set(w["choice"].tolist()) == {plp.PERSPECTIVE_CHOICE_NONE, plp.PERSPECTIVE_CHOICE_H, plp.PERSPECTIVE_CHOICE_F}
    assert w["status_f"][6] == INVALID and np.isnan(w["hyp_score_f"][6]).all() and np.isnan(w["rel_score_h"][6])
    assert w["status_h"][8] == w["status_f"][8] == INVALID
    check(mt, qs, seed=5, host=False)


def test_a_given_homography_mixed_with_ransac_problems(mt):
    """problem 0 hands in the matrix of a RANSAC run of its own (valid), 2 a matrix with too low a count, 3 one that fits nothing, 5 a singular one
    (all invalid), 4 has too few matches; the others run the H RANSAC in the same call"""
    qs = ragged()
    w = check(mt, qs, host=False)
    singular = np.outer([1.0, 2.0, 3.0], [0.5, -1.0, 2.0])
    given = {0: (w["H_21"][0], int(w["num_inliers_h"][0])), 3: (np.eye(3), 8), 2: (np.eye(3), 7), 5: (singular, 50), 4: (np.eye(3), 20)}
    g = check(mt, qs, given=given)
    assert g["status_h"][0] == OK and g["best_iter_h"][0] == -1 and same_bits(g["H_21"][0], w["H_21"][0]) and not g["hyp_score_h"][0].any()
    assert g["status_h"][[2, 3, 5]].tolist() == [INVALID] * 3 and g["status_h"][4] == FEW
    for k in ("status_f", "F_21", "score_f", "inliers_f", "hyp_score_f"):
        assert same_bits(g[k], w[k]), k                              # F is not affected
    for p in (1, 6, 7, 8, 9):
        assert same_bits(g["H_21"][p], w["H_21"][p]) and g["status_h"][p] == w["status_h"][p]


@pytest.mark.parametrize("recompute", [False, True])
@pytest.mark.parametrize("n_in", [8, 64, 65, 257])
def test_refit_over_inlier_counts_around_every_edge(mt, recompute, n_in):
    """six gross mismatches among n_in exact matches of a planar scene and samples of exact matches only: the best hypothesis of either solver has
    exactly n_in inliers"""
    q = S.problem(500 + n_in, n_in + 6, "perspective", n_slots=n_in + 20, noise=0.0, iters=8, kind="planar")
    slots = np.flatnonzero(q["match"] >= 0)
    is_out = np.zeros(n_in + 6, bool)
    is_out[[1, 3, n_in // 2, n_in, n_in + 2, n_in + 5]] = True
    rng = np.random.default_rng(n_in)
    for s in slots[is_out]:
        q["undist_2"]["x"][q["match"][s]] += 60.0 + 30.0 * rng.random()
        q["undist_2"]["y"][q["match"][s]] -= 50.0 + 30.0 * rng.random()
    good = np.flatnonzero(~is_out)
    for i in range(8):
        q["samples_h"][i] = rng.permutation(good)[:8]
        q["samples_f"][i] = rng.permutation(good)[:8]
    w = check(mt, [q], recompute=recompute)
    assert w["status_h"][0] == OK and w["num_inliers_h"][0] == n_in, w["num_inliers_h"]
    assert w["status_f"][0] == OK


def test_degenerate_samples(mt):
    q = S.degenerate_problem()
    w = check(mt, [q])
    for h in (w["hyp_score_h"][0], w["hyp_score_f"][0]):
        assert h[0] == 0 and h[1] == 0 and h[2] == 0 and h[3] == h[4], h
    assert w["best_iter_f"][0] >= 3 and w["best_iter_h"][0] != 5


def test_ties_between_lane_groups_waves_and_passes(mt):
    """the same sample at several iterations: equal scores in two lane groups of a workgroup of k_persp_hypotheses and two lanes of one of k_persp_count
    (3, 5), in two workgroups of the former (3, 20) and in two of both (3, 37); the lowest iteration wins"""
    q = S.problem(81, 90, "perspective", n_slots=100, noise=5e-4, mismatch=0.0, iters=40, kind="planar")
    w0 = check(mt, [q], recompute=False, host=False)
    for key, hyp, best in (("samples_h", "hyp_score_h", "best_iter_h"), ("samples_f", "hyp_score_f", "best_iter_f")):
        top = int(np.argmax(w0[hyp][0]))
        for i in (3, 5, 20, 37):
            q[key][i] = q[key][top]
        if top not in (3, 5, 20, 37):
            q[key][top] = q[key][(top + 1) % 40 if (top + 1) % 40 not in (3, 5, 20, 37) else (top + 2) % 40]
    w = check(mt, [q], recompute=False)
    for hyp, best in (("hyp_score_h", "best_iter_h"), ("hyp_score_f", "best_iter_f")):
        assert w[best][0] == 3 and len(set(w[hyp][0][[3, 5, 20, 37]].tolist())) == 1 and w[hyp][0].max() == w[hyp][0][3]


def test_optional_outputs_absent(mt):
    qs = [S.problem(91, 80, "perspective", n_slots=100, noise=1e-3), S.problem(92, 5, "fisheye")]
    check(mt, qs, skip_optional=True, host=False)


def test_two_calls_back_to_back_on_one_stream(mt):
    """the second call reuses the context's buffers behind the first on the same stream, with nothing synchronised in between"""
    import torch
    a1 = S.pack([S.problem(95, 130, "perspective", n_slots=160, noise=1e-3, mismatch=0.2), S.problem(96, 20, "perspective")])
    a2 = S.pack([S.problem(97, 64, "fisheye", n_slots=70, noise=1e-3, kind="planar")])
    o1, k1 = enqueue_device(mt, a1, True, None)
    o2, k2 = enqueue_device(mt, a2, True, 9)
    torch.cuda.synchronize()
    for a, o, seed in ((a1, o1, None), (a2, o2, 9)):
        P, n_cap = a["match"].shape
        pos, kw = S.call_kwargs(a, True, seed)
        want = plp.model_perspective_ransac(*pos, out=sentinels(P, n_cap, 24), **kw)
        for k in want:
            assert same_bits(o[k].cpu().numpy(), want[k]), k


def test_mirror_classes_on_the_device(mt):
    q = S.problem(99, 60, "perspective", n_slots=70, noise=5e-4, mismatch=0.2, kind="planar")
    pairs = [(s, int(m)) for s, m in enumerate(q["match"]) if m >= 0]
    for cls, key, get in ((plp.homography_solver, "samples_h", "get_best_H_21"), (plp.fundamental_solver, "samples_f", "get_best_F_21")):
        s = cls(q["undist_1"], q["undist_2"], pairs, 1.0, mt=mt, samples=q[key])
        s.find_via_ransac(24)
        m = cls(q["undist_1"], q["undist_2"], pairs, 1.0, samples=q[key])
        m.find_via_ransac(24)
        assert s.solution_is_valid() and m.solution_is_valid()
        assert same_bits(getattr(s, get)(), getattr(m, get)()) and same_bits(s.get_inlier_matches(), m.get_inlier_matches())
        assert s.get_best_score() == m.get_best_score() and len(s.get_inlier_matches()) == 60


def test_argument_checks_of_both_entries(mt):
    """a bad argument is refused before anything is written; P == 0 or n_cap == 0 writes nothing"""
    import torch
    a = S.pack([S.problem(1, 12, "perspective", iters=1)])
    pos = (a["undist_1"], a["undist_2"], a["match"])
    out = sentinels(1, 12, 1)
    with pytest.raises(plp.PlpError) as e:
        mt.perspective_ransac(*pos, iters=0, out=out)
    assert e.value.status == plp.PLP_ERR_INVALID_ARG and all((v == SENT[v.dtype]).all() for v in out.values())
    with pytest.raises(plp.PlpError) as e:
        mt.perspective_ransac(np.zeros((1, 8193), plp.KP_DTYPE), np.zeros((1, 4), plp.KP_DTYPE), np.zeros((1, 8193), np.int32))
    assert e.value.status == plp.PLP_ERR_UNSUPPORTED
    with pytest.raises(plp.PlpError) as e:
        mt.perspective_ransac(*pos, iters=1, given_H_21=np.eye(3)[None], out=out)
    assert e.value.status == plp.PLP_ERR_INVALID_ARG and all((v == SENT[v.dtype]).all() for v in out.values())
    o = {k: to_device(v) for k, v in sentinels(1, 12, 24).items()}
    dev = [to_device(v) for v in pos]
    m_cap = a["undist_2"].shape[1]
    with pytest.raises(plp.PlpError) as e:
        mt.perspective_ransac_device(1, 12, m_cap, *dev, o, iters=0)
    assert e.value.status == plp.PLP_ERR_INVALID_ARG
    with pytest.raises(plp.PlpError) as e:
        mt.perspective_ransac_device(1, 12, m_cap, dev[0], None, dev[2], o)
    assert e.value.status == plp.PLP_ERR_INVALID_ARG
    with pytest.raises(plp.PlpError) as e:
        mt.perspective_ransac_device(1, 12, m_cap, *dev, {k: v for k, v in o.items() if k != "choice"})
    assert e.value.status == plp.PLP_ERR_INVALID_ARG
    mt.perspective_ransac_device(0, 12, m_cap, *dev, o)                            # nothing to do
    mt.perspective_ransac_device(1, 0, 0, None, None, None, {})
    torch.cuda.synchronize()
    for k, v in o.items():
        assert (v.cpu().numpy() == SENT[np.dtype(plp.PERSPECTIVE_RANSAC_OUTPUTS[k][1])]).all(), k
