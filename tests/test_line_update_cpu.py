"""The line map update without a GPU: the host build of csrc/line_update.hpp (plp.model_trim_line_endpoints,
plp.model_correct_landmark_lines, plp.model_loop_ba_propagate_lines) against the plain-Python restatement tests/line_update_ref.py bit for bit, the
restatement against independent geometry (the true end points, the rigid motion of end points, numpy's matrix product), and the argument checks."""
import numpy as np
import pytest

import line_update_ref as R
import line_update_scene as S
from plp import plp

SCENES = dict(f5=dict(seed=1, F=5, n_lines=120), f13=dict(seed=2, F=13, n_lines=60), f1=dict(seed=3, F=1, n_lines=20), f3_stride17=dict(seed=4, F=3, n_lines=40, stride=17))
_cache = {}

# The largest deviations of the RESTATEMENT from ground truth / numpy over SCENES, measured with measure() below (python tests/test_line_update_cpu.py prints
# them), and the bounds the tests assert: ten times the measured value (D24's margin).  DESIGN.md D25 records the same numbers.
MEASURED = dict(trim_true_endpoints=3.255e-07, corr_vs_numpy=3.365e-16, corr_rigid_direction=7.448e-15, corr_rigid_moment=3.464e-14, prop_rigid_direction=2.625e-15,
                prop_rigid_moment=1.044e-14)
BOUND = {k: 10.0 * v for k, v in MEASURED.items()}


def scene(name):
    if name not in _cache:
        _cache[name] = S.scene(**SCENES[name])
    return _cache[name]


def sentinels(ref):
    return {k: np.full_like(v, R.SENTINEL[k]) for k, v in ref.items()}


# ---- the condition on the scenes, on the restatement alone
@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("mode", [R.TRIM_DEPTH_POSITIVE, R.TRIM_MAX_CHANGE])
def test_scene_keeps_most_lines_and_reaches_every_exit(name, mode):
    sc = scene(name)
    r = R.trim_line_endpoints(sc["cam"], **S.trim_kwargs(sc, mode))
    n = sc["undirected"]
    assert (r["status"][:n] == R.TRIM_OK).mean() >= 0.8
    st = {k: int(r["status"][i]) for k, i in sc["directed"].items()}
    depth = mode == R.TRIM_DEPTH_POSITIVE
    want = dict(erased=R.TRIM_SKIPPED, no_ref=R.TRIM_NO_REF, ref_outside=R.TRIM_NO_REF, ref_erased=R.TRIM_NO_REF, not_observing=R.TRIM_NOT_OBSERVED,
                idx_minus_one=R.TRIM_NOT_OBSERVED, idx_at_counts=R.TRIM_INDEX_RANGE,
                # a NaN compares false: `0 < z` rejects it, `change > 0.1` does not (D25)
                behind=R.TRIM_REJECTED if depth else R.TRIM_OK, horizontal=R.TRIM_REJECTED if depth else R.TRIM_OK,
                vertical=R.TRIM_REJECTED if depth else R.TRIM_OK, nan_pose=R.TRIM_REJECTED if depth else R.TRIM_OK,
                moved=R.TRIM_OK if depth else R.TRIM_REJECTED)
    assert st == want
    for k in ("horizontal", "vertical"):
        l1, l2, _ = R.reprojected_line(sc["cam"], [float(v) for v in sc["pose"][0]], [float(v) for v in sc["pluecker"][sc["directed"][k]]])
        assert (l1 == 0.0 and l2 != 0.0) if k == "horizontal" else (l2 == 0.0 and l1 != 0.0)
    erase = np.isin(r["status"], (R.TRIM_NOT_OBSERVED, R.TRIM_REJECTED)).astype(np.uint8)
    assert np.array_equal(r["erase"], erase)
    lens = np.diff(sc["obs_offsets"][:n + 1])
    assert lens.min() == 0 and 1 in lens and lens.max() == min(SCENES[name]["F"], 12)


# ---- the host build against the restatement, bit for bit
@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("mode", [R.TRIM_DEPTH_POSITIVE, R.TRIM_MAX_CHANGE])
@pytest.mark.parametrize("counts", [True, False])
def test_model_trim_equals_restatement(name, mode, counts):
    sc = scene(name)
    kw = S.trim_kwargs(sc, mode, counts)
    want = R.trim_line_endpoints(sc["cam"], **kw)
    got = plp.model_trim_line_endpoints(sc["camera"], **kw, out=sentinels(want))
    for k in want:
        assert S.same_bits(got[k], want[k]), k
    assert np.all(got["pos_w"][want["status"] != R.TRIM_OK] == R.SENTINEL["pos_w"])


def test_model_trim_in_place_and_without_key_lines():
    sc = scene("f5")
    kw = S.trim_kwargs(sc, R.TRIM_MAX_CHANGE)
    want = R.trim_line_endpoints(sc["cam"], **kw, out=dict(sentinels(R.trim_line_endpoints(sc["cam"], **kw)), pos_w=sc["pos_w_old"]))
    buf = sc["pos_w_old"].copy()
    got = plp.model_trim_line_endpoints(sc["camera"], **dict(kw, pos_w_old=buf), out=dict(sentinels(want), pos_w=buf))
    assert got["pos_w"] is buf
    for k in want:
        assert S.same_bits(got[k], want[k]), k
    # cap = 0: no key line can be reached
    kw0 = dict(S.trim_kwargs(sc, R.TRIM_DEPTH_POSITIVE, False), keylines=sc["keylines"][:, :0])
    want = R.trim_line_endpoints(sc["cam"], **kw0)
    got = plp.model_trim_line_endpoints(sc["camera"], **kw0, out=sentinels(want))
    assert set(np.unique(want["status"])) <= {R.TRIM_SKIPPED, R.TRIM_NO_REF, R.TRIM_NOT_OBSERVED, R.TRIM_INDEX_RANGE} and R.TRIM_INDEX_RANGE in want["status"]
    for k in want:
        assert S.same_bits(got[k], want[k]), k
    # L = 0
    e = plp.model_trim_line_endpoints(sc["camera"], np.zeros((0, 6)), np.zeros(0, np.int32), np.zeros(1, np.int32), [], [], sc["pose"], sc["keylines"])
    assert e["pos_w"].shape == (0, 6) and e["status"].shape == (0,)


@pytest.mark.parametrize("name", SCENES)
def test_model_correct_landmark_lines_equals_restatement(name):
    sc = scene(name)
    for kw in (S.correct_case(sc, 5), dict(S.correct_case(sc, 6), corr_kf=None, lm_erased=None)):
        want = R.correct_landmark_lines(**kw)
        got = plp.model_correct_landmark_lines(**kw, out=sentinels(want))
        assert set(np.unique(want["status"])) >= {R.CORRECT_LINE_OK, R.CORRECT_LINE_NO_REF}
        for k in want:
            assert S.same_bits(got[k], want[k]), k


@pytest.mark.parametrize("name", SCENES)
def test_model_loop_ba_propagate_lines_equals_restatement(name):
    sc = scene(name)
    for kw in (S.propagate_case(sc, 7), dict(S.propagate_case(sc, 8), line_optimized=None, pluecker_after=None)):
        want = R.loop_ba_propagate_lines(**kw)
        got = plp.model_loop_ba_propagate_lines(**kw, out=sentinels(want))
        assert R.LM_MOVED in want["status"] and R.LM_ERASED in want["status"]
        for k in want:
            assert S.same_bits(got[k], want[k]), k


def test_non_finite_sim3_reaches_every_sum():
    """the zero blocks of the 6 x 6 matrices are multiplied, not skipped: an infinite scale turns the whole product into NaN (0 * inf in
    the lower left block), an infinite tx the two rows skew(t) carries it into, in both builds alike"""
    rng = np.random.default_rng(9)
    cw, wc = S.random_sim3(rng, 3)
    cw[1, 7] = np.inf
    wc[2, 4] = np.inf
    kw = dict(pluecker=rng.normal(0, 1, (3, 6)), ref_kf=np.array([0, 1, 2], np.int32), sim3_cw=cw, corrected_wc=wc)
    want = R.correct_landmark_lines(**kw)
    got = plp.model_correct_landmark_lines(**kw)
    assert np.all(np.isfinite(want["pluecker"][0])) and np.all(np.isnan(want["pluecker"][1])) and np.all(np.isnan(want["pluecker"][2, 1:3]))
    assert S.same_bits(got["pluecker"], want["pluecker"])


# ---- the restatement against independent geometry
def _as_line(L6):
    """(unit direction, m / |d|) with the sign fixed by the direction's largest component"""
    d = L6[3:] / np.linalg.norm(L6[3:])
    m = L6[:3] / np.linalg.norm(L6[3:])
    s = np.sign(d[np.argmax(np.abs(d))])
    return s * d, s * m


def _line_deviation(got6, sp, ep):
    d, m = _as_line(got6)
    dr, mr = _as_line(S.pluecker_of(sp, ep))
    return float(np.linalg.norm(np.cross(d, dr))), float(np.max(np.abs(m - mr)))


def measure():
    out = {k: 0.0 for k in MEASURED}
    for name in SCENES:
        sc = scene(name)
        n = sc["undirected"]
        r = R.trim_line_endpoints(sc["cam"], **S.trim_kwargs(sc, R.TRIM_DEPTH_POSITIVE))
        clean = np.array([SCENES[name].get("noise_every", 4) == 0 or l % 4 != 1 for l in range(n)]) & (r["status"][:n] == R.TRIM_OK)
        out["trim_true_endpoints"] = max(out["trim_true_endpoints"], float(np.max(np.abs(r["pos_w"][:n][clean] - sc["true_pos_w"][:n][clean]))))
        # item 3 against numpy's product of the two 6 x 6 matrices, and with s = 1 against the rigid motion of the end points
        kw = S.correct_case(sc, 5)
        c = R.correct_landmark_lines(**kw)
        kw1 = dict(kw, sim3_cw=kw["sim3_cw"].copy(), corrected_wc=kw["corrected_wc"].copy())
        kw1["sim3_cw"][:, 7] = 1.0
        kw1["corrected_wc"][:, 7] = 1.0
        c1 = R.correct_landmark_lines(**kw1)
        for l in np.flatnonzero(c["status"] == R.CORRECT_LINE_OK):
            k = int(kw["corr_kf"][l])
            X, Y = np.array(R.sim3_transform6(kw["corrected_wc"][k])), np.array(R.sim3_transform6(kw["sim3_cw"][k]))
            ref = (X @ Y) @ sc["pluecker"][l]
            out["corr_vs_numpy"] = max(out["corr_vs_numpy"], float(np.max(np.abs(c["pluecker"][l] - ref) / np.linalg.norm(ref))))
            Rc, tc = _rt(kw1["sim3_cw"][k])
            Rw, tw = _rt(kw1["corrected_wc"][k])
            sp, ep = (Rw @ (Rc @ p + tc) + tw for p in (sc["true_pos_w"][l, :3], sc["true_pos_w"][l, 3:]))
            dd, dm = _line_deviation(c1["pluecker"][l], sp, ep)
            out["corr_rigid_direction"], out["corr_rigid_moment"] = max(out["corr_rigid_direction"], dd), max(out["corr_rigid_moment"], dm)
        kw = S.propagate_case(sc, 7)
        p = R.loop_ba_propagate_lines(**kw)
        for l in np.flatnonzero(p["status"] == R.LM_MOVED):
            k = int(kw["ref_kf"][l])
            b, a = kw["pose_before"][k], kw["pose_after"][k]
            Rb, tb, Ra, ta = b[:9].reshape(3, 3), b[9:12], a[:9].reshape(3, 3), a[9:12]
            sp, ep = (Ra.T @ ((Rb @ q + tb) - ta) for q in (sc["true_pos_w"][l, :3], sc["true_pos_w"][l, 3:]))
            dd, dm = _line_deviation(p["pluecker"][l], sp, ep)
            out["prop_rigid_direction"], out["prop_rigid_moment"] = max(out["prop_rigid_direction"], dd), max(out["prop_rigid_moment"], dm)
    return out


def _rt(sim3):
    import pose_optimizer_ref as D15
    return np.array(D15.rot_from_quat([float(v) for v in sim3[:4]])).reshape(3, 3), np.asarray(sim3[4:7], np.float64)


def test_restatement_agrees_with_independent_geometry():
    got = measure()
    print(got)
    for k, v in got.items():
        assert v <= BOUND[k], (k, v, BOUND[k])


# ---- argument checks: the code, and nothing written
def test_refused_calls_return_their_code_and_write_nothing():
    sc = scene("f5")
    kw = S.trim_kwargs(sc, R.TRIM_MAX_CHANGE)
    blank = sentinels(R.trim_line_endpoints(sc["cam"], **kw))

    def refused(status, fn, *a, **k):
        out = {n: v.copy() for n, v in blank.items()} if "pos_w" in k.get("out", {}) else None
        if out is not None:
            k["out"] = out
        with pytest.raises(plp.PlpError) as e:
            fn(*a, **k)
        assert e.value.status == status, (e.value, status)
        if out is not None:
            assert all(np.array_equal(out[n], blank[n]) for n in out)
    cam = sc["camera"]
    for model, status in ((plp.CAMERA_FISHEYE, plp.PLP_ERR_UNSUPPORTED), (plp.CAMERA_EQUIRECTANGULAR, plp.PLP_ERR_UNSUPPORTED), (7, plp.PLP_ERR_INVALID_ARG)):
        bad = S.camera()
        bad.model = model
        refused(status, plp.model_trim_line_endpoints, bad, **kw, out=blank)
    for field, v in (("fx", 0.0), ("fy", float("nan")), ("cx", float("inf"))):
        bad = S.camera()
        setattr(bad, field, v)
        refused(plp.PLP_ERR_INVALID_ARG, plp.model_trim_line_endpoints, bad, **kw, out=blank)
    refused(plp.PLP_ERR_INVALID_ARG, plp.model_trim_line_endpoints, cam, **dict(kw, mode=2), out=blank)
    refused(plp.PLP_ERR_INVALID_ARG, plp.model_trim_line_endpoints, cam, **dict(kw, pos_w_old=None), out=blank)
    refused(plp.PLP_ERR_INVALID_ARG, plp.model_trim_line_endpoints, cam, **dict(kw, median_depth=None), out=blank)
    refused(plp.PLP_ERR_INVALID_ARG, plp.model_trim_line_endpoints, cam, **dict(kw, pose=sc["pose"][:, :11]), out=blank)
    down = sc["obs_offsets"].copy()
    down[3] = down[2] - 1
    refused(plp.PLP_ERR_INVALID_ARG, plp.model_trim_line_endpoints, cam, **dict(kw, obs_offsets=down), out=blank)
    up = sc["obs_offsets"] + 1
    refused(plp.PLP_ERR_INVALID_ARG, plp.model_trim_line_endpoints, cam, **dict(kw, obs_offsets=up, obs_kf=np.append(sc["obs_kf"], 0), obs_idx=np.append(sc["obs_idx"], 0)),
            out=blank)
    # the two transforms: the table limits of the optimisers they follow
    rng = np.random.default_rng(1)
    cw, wc = S.random_sim3(rng, plp.POSE_GRAPH_MAX_KF + 1)
    refused(plp.PLP_ERR_UNSUPPORTED, plp.model_correct_landmark_lines, np.zeros((2, 6)), np.zeros(2, np.int32), cw, wc)
    F = plp.GLOBAL_BA_MAX_KF + 1
    refused(plp.PLP_ERR_UNSUPPORTED, plp.model_loop_ba_propagate_lines, np.zeros((F, 15)), np.zeros((F, 12)), np.zeros(F, np.uint8), np.zeros((2, 6)), np.zeros(2, np.int32))
    refused(plp.PLP_ERR_INVALID_ARG, plp.model_loop_ba_propagate_lines, np.zeros((2, 15)), np.zeros((2, 12)), np.zeros(2, np.uint8), np.zeros((2, 6)), np.zeros(2, np.int32),
            line_optimized=np.ones(2, np.uint8))


if __name__ == "__main__":
    for k, v in measure().items():
        print(f"{k}: {v:.3e}")
