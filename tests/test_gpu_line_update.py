"""The line map update on the device (plp_trim_line_endpoints_*, plp_correct_landmark_lines_*, plp_loop_ba_propagate_lines_*, csrc/line_update_kernels.hip;
DESIGN.md section 5, D25) against the CPU build of the same header (plp.model_*, which tests/test_line_update_cpu.py holds bit for bit to the restatement
tests/line_update_ref.py): every output bit for bit on sentinel-filled arrays, through the device entry and the staged host-pointer entry, at the smallest
shapes at which the kernels can go wrong -- one lane per line in workgroups of 256 lanes (BLOCK): line counts around one workgroup and above two, one key
frame and several, no key-line slot at all, counts absent and ragged, the end points written over the old ones."""
import numpy as np
import pytest

import global_ba_scene as GS
import line_update_ref as R
import line_update_scene as S
from plp import plp

pytestmark = pytest.mark.gpu
BLOCK = 256
N = lambda t: t.cpu().numpy()
_cache = {}


@pytest.fixture(scope="module")
def mt():
    return plp.matcher()


def dev(v):
    import torch
    v = np.ascontiguousarray(v)
    if v.dtype.fields and v.size == 0:
        return torch.zeros(v.shape + (v.dtype.itemsize,), dtype=torch.uint8, device="cuda")
    return torch.from_numpy((v.view(np.uint8).reshape(v.shape + (-1,)) if v.dtype.fields else v).copy()).cuda()


def scene(F, L):
    """L lines over F live key frames: the directed rows first, undirected ones behind them"""
    if (F, L) not in _cache:
        sc = S.scene(100 + F, F=F, n_lines=max(L, 13))
        n, D = sc["undirected"], len(S.DIRECTED)
        idx = list(range(n, n + D)) + list(range(n))
        _cache[F, L] = S.take(sc, idx[:L] if L > 1 else [1])
    return _cache[F, L]


def sentinels(want):
    return {k: np.full_like(v, R.SENTINEL[k]) for k, v in want.items()}


def check_trim(mt, sc, mode, counts=True, alias=False, keylines=None):
    import torch
    kw = S.trim_kwargs(sc, mode, counts)
    if keylines is not None:
        kw["keylines"] = keylines
    L, F, cap = len(sc["pluecker"]), len(sc["pose"]), kw["keylines"].shape[1]
    blank = sentinels(dict(pos_w=np.zeros((L, 6)), status=np.zeros(L, np.uint8), erase=np.zeros(L, np.uint8)))
    if alias:
        blank["pos_w"] = sc["pos_w_old"].copy()
    want = plp.model_trim_line_endpoints(sc["camera"], **(dict(kw, pos_w_old=blank["pos_w"]) if alias else kw), out=blank)
    o = {k: dev(sc["pos_w_old"] if alias and k == "pos_w" else np.full_like(v, R.SENTINEL[k])) for k, v in want.items()}
    d = {k: None if v is None else dev(v) for k, v in kw.items() if k not in ("mode",)}
    if alias:
        d["pos_w_old"] = o["pos_w"]
    mt.trim_line_endpoints_device(sc["camera"], L, F, cap, d["pluecker"], d["ref_kf"], d["obs_offsets"], d["obs_kf"] if d["obs_kf"].numel() else None,
                                  d["obs_idx"] if d["obs_idx"].numel() else None, d["pose"], d["keylines"] if cap else None, o["pos_w"], o["status"], o["erase"],
                                  mode=mode, skip=d["skip"], kf_erased=d["kf_erased"], counts=d["counts"], pos_w_old=d.get("pos_w_old"),
                                  median_depth=d.get("median_depth"), pose_stride=sc["pose"].shape[1])
    torch.cuda.synchronize()
    for k in want:
        assert S.same_bits(N(o[k]), want[k]), ("device", k)
    # the staged entry: the same kernel over host arrays
    out = {k: (sc["pos_w_old"].copy() if alias and k == "pos_w" else np.full_like(v, R.SENTINEL[k])) for k, v in want.items()}
    got = mt.trim_line_endpoints(sc["camera"], **(dict(kw, pos_w_old=out["pos_w"]) if alias else kw), out=out)
    for k in want:
        assert S.same_bits(got[k], want[k]), ("host", k)
    return want


@pytest.mark.parametrize("L", [1, BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK + 77])
@pytest.mark.parametrize("mode", [R.TRIM_DEPTH_POSITIVE, R.TRIM_MAX_CHANGE])
def test_trim_line_counts_around_a_workgroup(mt, L, mode):
    want = check_trim(mt, scene(5, L), mode)
    if L > 1:
        assert set(want["status"].tolist()) == {R.TRIM_OK, R.TRIM_SKIPPED, R.TRIM_NO_REF, R.TRIM_NOT_OBSERVED, R.TRIM_INDEX_RANGE, R.TRIM_REJECTED}
        assert (want["status"] == R.TRIM_OK).sum() >= (L - len(S.DIRECTED)) * 0.8


@pytest.mark.parametrize("mode", [R.TRIM_DEPTH_POSITIVE, R.TRIM_MAX_CHANGE])
@pytest.mark.parametrize("counts", [True, False])
def test_trim_one_key_frame_counts_absent_and_ragged(mt, mode, counts):
    check_trim(mt, scene(1, 40), mode, counts=counts)
    check_trim(mt, scene(5, BLOCK + 1), mode, counts=counts)


@pytest.mark.parametrize("counts", [True, False])
def test_trim_without_key_line_slots(mt, counts):
    sc = scene(5, BLOCK + 1)
    want = check_trim(mt, sc, R.TRIM_DEPTH_POSITIVE, counts=counts, keylines=sc["keylines"][:, :0])
    assert set(want["status"].tolist()) == {R.TRIM_SKIPPED, R.TRIM_NO_REF, R.TRIM_NOT_OBSERVED, R.TRIM_INDEX_RANGE}


def test_trim_writes_over_the_old_end_points(mt):
    sc = scene(5, 2 * BLOCK + 77)
    want = check_trim(mt, sc, R.TRIM_MAX_CHANGE, alias=True)
    kept = want["status"] != R.TRIM_OK
    assert kept.any() and np.array_equal(want["pos_w"][kept], sc["pos_w_old"][kept])


def test_no_line_is_ok_and_writes_nothing(mt):
    import torch
    sc = scene(5, BLOCK)
    o = dict(pos_w=dev(np.full((4, 6), -7.25)), status=dev(np.full(4, 0xEE, np.uint8)), erase=dev(np.full(4, 0x77, np.uint8)))
    mt.trim_line_endpoints_device(sc["camera"], 0, len(sc["pose"]), sc["keylines"].shape[1], None, None, None, None, None, dev(sc["pose"]), dev(sc["keylines"]),
                                  o["pos_w"], o["status"], o["erase"])
    mt.correct_landmark_lines_device(0, 3, None, None, None, None, o["pos_w"], o["status"])
    mt.loop_ba_propagate_lines_device(0, 3, None, None, None, None, None, o["pos_w"], o["status"])
    torch.cuda.synchronize()
    assert (N(o["pos_w"]) == -7.25).all() and (N(o["status"]) == 0xEE).all() and (N(o["erase"]) == 0x77).all()
    e = mt.trim_line_endpoints(sc["camera"], np.zeros((0, 6)), np.zeros(0, np.int32), np.zeros(1, np.int32), [], [], sc["pose"], sc["keylines"])
    assert e["status"].shape == (0,)


def test_refused_device_calls_write_nothing(mt):
    import torch
    sc = scene(5, BLOCK)
    L = len(sc["pluecker"])
    o = dict(pos_w=dev(np.full((L, 6), -7.25)), status=dev(np.full(L, 0xEE, np.uint8)), erase=dev(np.full(L, 0x77, np.uint8)))
    d = {k: dev(sc[k]) for k in ("pluecker", "ref_kf", "obs_offsets", "obs_kf", "obs_idx", "pose", "keylines")}
    bad = S.camera()
    bad.model = plp.CAMERA_FISHEYE
    for cam, kw, status in ((bad, {}, plp.PLP_ERR_UNSUPPORTED), (sc["camera"], dict(mode=R.TRIM_MAX_CHANGE), plp.PLP_ERR_INVALID_ARG),
                            (sc["camera"], dict(pose_stride=11), plp.PLP_ERR_INVALID_ARG)):
        with pytest.raises(plp.PlpError) as e:
            mt.trim_line_endpoints_device(cam, L, len(sc["pose"]), sc["keylines"].shape[1], d["pluecker"], d["ref_kf"], d["obs_offsets"], d["obs_kf"], d["obs_idx"],
                                          d["pose"], d["keylines"], o["pos_w"], o["status"], o["erase"], **kw)
        assert e.value.status == status
    torch.cuda.synchronize()
    assert (N(o["pos_w"]) == -7.25).all() and (N(o["status"]) == 0xEE).all() and (N(o["erase"]) == 0x77).all()


# ---- the two transforms, fed by the optimisers' own outputs on the device
@pytest.mark.parametrize("L", [1, BLOCK - 1, BLOCK + 1, 2 * BLOCK + 77])
def test_correct_landmark_lines_after_a_real_pose_graph(mt, L):
    import torch
    import test_gpu_loop_correction_step as LC
    import test_gpu_pose_graph as PG
    t, prs, _, _ = LC.scene()
    F = len(t["kf_parent"])
    o, keep = PG.enqueue_device(mt, t, prs, 64, 512)
    _, _, ln = S.map_lines(31, t["pose"], t["kf_erased"], L)
    rng = np.random.default_rng(L)
    corr = ln["ref_kf_lines"].copy()
    corr[::7] = rng.integers(-1, F + 1, len(corr[::7]))
    out = dict(pluecker=dev(np.full((L, 6), R.SENTINEL["pluecker"])), status=dev(np.full(L, R.SENTINEL["status"], np.uint8)))
    mt.correct_landmark_lines_device(L, F, dev(ln["pluecker_lines"]), dev(ln["ref_kf_lines"]), o["sim3_cw"], o["corrected_wc"], out["pluecker"], out["status"],
                                     corr_kf=dev(corr), lm_erased=dev(ln["skip_lines"]), kf_erased=dev(t["kf_erased"]))
    torch.cuda.synchronize()
    assert N(o["status"])[0] == plp.POSE_GRAPH_OK
    cw, wc = N(o["sim3_cw"])[0], N(o["corrected_wc"])[0]
    kw = dict(pluecker=ln["pluecker_lines"], ref_kf=ln["ref_kf_lines"], sim3_cw=cw, corrected_wc=wc, corr_kf=corr, lm_erased=ln["skip_lines"], kf_erased=t["kf_erased"])
    want = plp.model_correct_landmark_lines(**kw, out=sentinels(dict(pluecker=np.zeros((L, 6)), status=np.zeros(L, np.uint8))))
    if L > BLOCK:
        assert set(want["status"].tolist()) == {R.CORRECT_LINE_OK, R.CORRECT_LINE_ERASED, R.CORRECT_LINE_NO_REF, R.CORRECT_LINE_NO_VERTEX}
        ok = want["status"] == R.CORRECT_LINE_OK
        assert (want["pluecker"][ok] != ln["pluecker_lines"][ok]).any()
    for k in want:
        assert S.same_bits(N(out[k]), want[k]), ("device", k)
    got = mt.correct_landmark_lines(**kw, out=sentinels(want))
    for k in want:
        assert S.same_bits(got[k], want[k]), ("host", k)
    # in place
    pk = dev(ln["pluecker_lines"])
    mt.correct_landmark_lines_device(L, F, pk, dev(ln["ref_kf_lines"]), o["sim3_cw"], o["corrected_wc"], pk, out["status"], corr_kf=dev(corr),
                                     lm_erased=dev(ln["skip_lines"]), kf_erased=dev(t["kf_erased"]))
    torch.cuda.synchronize()
    ok = want["status"] == R.CORRECT_LINE_OK
    assert S.same_bits(N(pk), np.where(ok[:, None], want["pluecker"], ln["pluecker_lines"]))


@pytest.mark.parametrize("tree", ["deep", "erased", "broken"])
@pytest.mark.parametrize("L", [1, BLOCK + 1, 2 * BLOCK + 77])
def test_loop_ba_propagate_lines_after_a_real_propagation(mt, tree, L):
    import torch
    tr = GS.tree(tree)
    F, Lp = len(tr["pose"]), len(tr["pos_w"])
    pr = dict(pose=dev(tr["pose"]), pose_before=dev(tr["pose"][:, :12]), kf_status=dev(np.zeros(F, np.uint8)), pos_w=dev(tr["pos_w"]), lm_status=dev(np.zeros(Lp, np.uint8)))
    mt.loop_ba_propagate_device(F, Lp, dev(tr["pose"]), dev(tr["kf_parent"]), dev(tr["kf_optimized"]), dev(tr["pose_after"]), dev(tr["pos_w"]), dev(tr["ref_kf"]),
                                dev(tr["lm_optimized"]), dev(tr["pos_after"]), pr, kf_erased=dev(tr["kf_erased"]), kf_is_origin=dev(tr["kf_is_origin"]),
                                lm_erased=dev(tr["lm_erased"]), pose_stride=tr["pose"].shape[1])
    _, _, ln = S.map_lines(41, tr["pose"], tr["kf_erased"], L)
    rng = np.random.default_rng(L)
    opt = (rng.uniform(size=L) < 0.3).astype(np.uint8)
    after = ln["pluecker_lines"] + rng.normal(0, 0.01, (L, 6))
    out = dict(pluecker=dev(np.full((L, 6), R.SENTINEL["pluecker"])), status=dev(np.full(L, R.SENTINEL["status"], np.uint8)))
    mt.loop_ba_propagate_lines_device(L, F, pr["pose"], pr["pose_before"], pr["kf_status"], dev(ln["pluecker_lines"]), dev(ln["ref_kf_lines"]), out["pluecker"],
                                      out["status"], line_optimized=dev(opt), pluecker_after=dev(after), lm_erased=dev(ln["skip_lines"]))
    torch.cuda.synchronize()
    kw = dict(pose_after=N(pr["pose"]), pose_before=N(pr["pose_before"]), kf_status=N(pr["kf_status"]), pluecker=ln["pluecker_lines"], ref_kf=ln["ref_kf_lines"],
              line_optimized=opt, pluecker_after=after, lm_erased=ln["skip_lines"])
    want = plp.model_loop_ba_propagate_lines(**kw, out=sentinels(dict(pluecker=np.zeros((L, 6)), status=np.zeros(L, np.uint8))))
    if L > BLOCK:
        assert {R.LM_OPTIMIZED, R.LM_MOVED, R.LM_ERASED} <= set(want["status"].tolist())
    for k in want:
        assert S.same_bits(N(out[k]), want[k]), ("device", k)
    got = mt.loop_ba_propagate_lines(**kw, out=sentinels(want))
    for k in want:
        assert S.same_bits(got[k], want[k]), ("host", k)
