"""optimize::local_bundle_adjuster on the device (plp_local_ba_device / _host, csrc/local_ba_kernels.hip) against the CPU build of the same header
(plp.model_local_ba, which tests/test_local_ba_cpu.py holds bit for bit to the restatement tests/local_ba_ref.py): every
output bit for bit on sentinel-filled arrays, at the smallest shapes at which the kernels can go wrong.  The widths the kernels use: the workgroup
of 512 lanes (TEAM: the stride of every loop over observation entries, landmarks, key frames and work items, and the LDS tile of the chains over
the landmarks), the wave of 64 (WAVE: the ballot scans over the observation entries), 27 pose-sum items and 42 Schur items per free key frame
against TEAM, and one lane per row of the reduced system, whose 6 rows per free key frame cross a wave at 11 free key frames.  There is no list of
block pairs in this build (D17 item 8): the Schur items take its place at the boundaries."""
import numpy as np
import pytest

import local_ba_scene as S
from plp import plp

pytestmark = pytest.mark.gpu
TEAM, WAVE = 512, 64       # kLaThreads of csrc/local_ba.hpp and the wave size
OPTIONAL = ("round_info", "round_chi2")
TABLES = ("pose", "kf_erased", "kf_is_origin", "undist", "x_right", "counts", "pos_w", "lm_erased", "obs_offsets", "obs_kf", "obs_idx")


@pytest.fixture(scope="module")
def mt():
    return plp.matcher()


def dims(sc):
    return len(sc["pose"]), len(sc["pos_w"]), len(sc["obs_kf"])


def cut(sc, T):
    """the scene with its observation list cut to T entries (the landmarks behind them go)"""
    sc = dict(sc)
    L = int(np.searchsorted(sc["obs_offsets"], T, side="left"))
    assert 0 < L < len(sc["obs_offsets"]) and sc["obs_offsets"][L] >= T
    oo = sc["obs_offsets"][:L + 1].copy(); oo[L] = T
    sc.update(obs_offsets=oo, obs_kf=sc["obs_kf"][:T], obs_idx=sc["obs_idx"][:T], label=sc["label"][:T], pos_w=sc["pos_w"][:L], pos_gt=sc["pos_gt"][:L], lm_erased=sc["lm_erased"][:L])
    return sc


def host_model(sc, kf_local, **kw):
    F, L, T = dims(sc)
    G = len(kf_local)
    return plp.model_local_ba(**S.call_args(sc, kf_local=kf_local, **kw), out=S.sentinel_out(G, F, L, T))


def enqueue_device(mt, sc, kf_local, skip_optional=False, stream=None, keep=None, G=None, **kw):
    """plp_local_ba_device on sentinel-filled device outputs; returns the output tensors (nothing is synchronised).  keep: a dict that receives the
    output tensors before the call, for a call that is expected to raise; G: the G of the call when it is not the number of kf_local rows"""
    import torch
    F, L, T = dims(sc)
    rows = len(kf_local)
    G = rows if G is None else G

    def d(v):
        if v is None:
            return None
        v = np.ascontiguousarray(v)
        return torch.from_numpy((v.view(np.uint8) if v.dtype.fields else v).copy()).cuda()
    a = S.call_args(sc, kf_local=kf_local, **kw)
    o = {k: d(v) for k, v in S.sentinel_out(rows, F, L, T).items()}
    if keep is not None:
        keep.update(o)
    passed = {k: v for k, v in o.items() if not (skip_optional and k in OPTIONAL) and v.numel()}
    dev = {k: d(a[k]) for k in TABLES}
    dev["kf_local"] = d(np.ascontiguousarray(kf_local, np.uint8))
    mt.local_ba_device(a["camera"], a["setup_type"], G, F, L, T, sc["undist"].shape[1], dev["pose"], dev["undist"], dev["pos_w"], dev["obs_offsets"], dev["obs_kf"],
                       dev["obs_idx"], dev["kf_local"], a["inv_level_sigma_sq"], passed, x_right=dev["x_right"], counts=dev["counts"], kf_erased=dev["kf_erased"],
                       kf_is_origin=dev["kf_is_origin"], lm_erased=dev["lm_erased"], pose_stride=sc["pose"].shape[1], num_first_iter=a.get("num_first_iter", 5),
                       num_second_iter=a.get("num_second_iter", 10), stream=stream)
    return o, dev


def check(mt, sc, kf_local=None, skip_optional=False, **kw):
    import torch
    kf_local = sc["kf_local"][None] if kf_local is None else np.asarray(kf_local, np.uint8)
    want = host_model(sc, kf_local, **kw)
    o, _ = enqueue_device(mt, sc, kf_local, skip_optional=skip_optional, **kw)
    torch.cuda.synchronize()
    sent = S.sentinel_out(*((len(kf_local),) + dims(sc)))
    for k in want:
        got = o[k].cpu().numpy()
        ref = sent[k] if (skip_optional and k in OPTIONAL) else want[k]
        assert S.same({k: got}, {k: ref}), k
    return want


@pytest.mark.parametrize("T", [WAVE - 1, WAVE, WAVE + 1, TEAM - 1, TEAM, TEAM + 1])
def test_observation_counts_around_the_wave_and_the_team(mt, T):
    sc = cut(S.make_scene(100 + T, 3, 2, 200, setup=S.RGBD, noise=0.8, outliers=8, obs_share=0.7), T)
    want = check(mt, sc)
    assert want["status"][0] == plp.LOCAL_BA_OK and (want["outlier"][0] != 77).sum() > T // 2 and (T < TEAM - 1 or (want["outlier"][0] == 1).any())


@pytest.mark.parametrize("L", [TEAM - 1, TEAM, TEAM + 1])
def test_landmark_counts_around_the_team(mt, L):
    sc = S.make_scene(200 + L, 2, 2, L, noise=0.8, outliers=10, obs_share=0.4, n_other=1)
    want = check(mt, sc)
    assert want["lm_role"][0].sum() >= 300 and want["lm_role"][0][TEAM - 2:].any()          # the table, not the local set, is what the loops stride over


@pytest.mark.parametrize("n_free", [1, 2, 10, 11, 12, 13, 18, 19])
def test_free_key_frames_at_the_ownership_boundaries(mt, n_free):
    """10 / 11: the reduced system's rows cross a wave (60 / 66); 12 / 13: the Schur items cross the team (504 / 546); 18 / 19: the pose-sum items (486 / 513)"""
    sc = S.make_scene(300 + n_free, n_free, 2, 40, setup=S.RGBD, noise=0.8, outliers=4)
    want = check(mt, sc)
    assert (want["kf_role"][0] == plp.LOCAL_BA_KF_FREE).sum() == n_free and want["round_info"][0, 0, 0] == 5


def test_the_minimal_problem(mt):
    sc = S.make_scene(401, 1, 1, 5, noise=0.5, n_other=0, obs_share=1.0)
    want = check(mt, sc)
    assert dims(sc) == (2, 5, 10) and want["status"][0] == plp.LOCAL_BA_OK


@pytest.mark.parametrize("setup,model", [(S.MONO, "perspective"), (S.RGBD, "fisheye")])
def test_ragged_problems_over_shared_tables(mt, setup, model):
    """G = 3: a full problem, an empty one, and one whose only local key frame is the origin (no free pose); erased key frames and landmarks"""
    sc = S.make_scene(410, 3, 2, 50, model=model, setup=setup, noise=0.8, outliers=5, origin=True, n_other=2)
    sc["lm_erased"][[3, 17]] = 1
    F = len(sc["pose"])
    kl = np.zeros((3, F), np.uint8)
    kl[0] = sc["kf_local"]; kl[2, 0] = 1
    want = check(mt, sc, kl)
    assert want["status"].tolist() == [plp.LOCAL_BA_OK, plp.LOCAL_BA_NO_EDGES, plp.LOCAL_BA_OK]
    assert (want["kf_role"][2] == plp.LOCAL_BA_KF_FREE).sum() == 0 and (want["kf_role"][2] == plp.LOCAL_BA_KF_ORIGIN).sum() == 1
    assert (want["lm_role"][0, [3, 17]] == 0).all() and (want["pose"][1] == -7.5).all()


def test_odd_strides_and_absent_optionals(mt):
    sc = S.make_scene(420, 3, 2, 40, noise=0.8, outliers=3, kp_stride=61, pose_stride=13)
    assert sc["x_right"] is None
    sc.update(counts=None, kf_erased=None, kf_is_origin=None, lm_erased=None)
    check(mt, sc, skip_optional=True)


def test_both_iteration_counts_at_one(mt):
    sc = S.make_scene(430, 3, 2, 40, setup=S.STEREO, noise=0.8, outliers=4)
    want = check(mt, sc, num_first_iter=1, num_second_iter=1)
    assert want["round_info"][0, :, 0].tolist() == [1, 1]


@pytest.mark.parametrize("name", ["no_information", "nan", "behind", "seen_once"])
def test_the_census_scenes_that_fail_solves_and_drop_vertices(mt, name):
    check(mt, S.census()[name])


def test_two_calls_back_to_back_on_one_stream(mt):
    import torch
    a = S.make_scene(440, 3, 2, 60, setup=S.RGBD, noise=0.8, outliers=5)
    b = S.make_scene(441, 2, 1, 30, noise=0.8)
    wa, wb = host_model(a, a["kf_local"][None]), host_model(b, b["kf_local"][None])
    oa, keep_a = enqueue_device(mt, a, a["kf_local"][None])
    ob, keep_b = enqueue_device(mt, b, b["kf_local"][None])
    torch.cuda.synchronize()
    for want, o in ((wa, oa), (wb, ob)):
        for k in want:
            assert S.same({k: o[k].cpu().numpy()}, {k: want[k]}), k


def test_the_host_entry_equals_the_device_entry(mt):
    sc = S.make_scene(450, 3, 2, 40, setup=S.RGBD, noise=0.8, outliers=4)
    F, L, T = dims(sc)
    want = host_model(sc, sc["kf_local"][None])
    got = mt.local_ba(**S.call_args(sc, kf_local=sc["kf_local"][None]), out=S.sentinel_out(1, F, L, T))
    for k in want:
        assert S.same({k: got[k]}, {k: want[k]}), k
    one = plp.local_bundle_adjuster(mt=mt).optimize(**S.call_args(sc))
    assert S.same({"pose": one["pose"][want["kf_role"][0] == 1]}, {"pose": want["pose"][0][want["kf_role"][0] == 1]})


def test_refusals_write_nothing(mt):
    import torch
    sc = S.make_scene(460, 2, 1, 20, noise=0.5)
    F, L, T = dims(sc)
    eq = S.PS.camera("perspective"); eq.model = plp.CAMERA_EQUIRECTANGULAR
    out = S.sentinel_out(1, F, L, T)
    with pytest.raises(plp.PlpError) as e:
        mt.local_ba(**{**S.call_args(sc, kf_local=sc["kf_local"][None]), "camera": eq}, out=out)
    assert e.value.status == plp.PLP_ERR_UNSUPPORTED and S.same(out, S.sentinel_out(1, F, L, T))
    bad = dict(sc); bad["camera"] = eq
    sent = S.sentinel_out(1, F, L, T)
    kept = {}
    with pytest.raises(plp.PlpError) as e:
        enqueue_device(mt, bad, sc["kf_local"][None], keep=kept)
    torch.cuda.synchronize()
    assert e.value.status == plp.PLP_ERR_UNSUPPORTED and len(kept) == len(sent)
    for k in sent:
        assert S.same({k: kept[k].cpu().numpy()}, {k: sent[k]}), k
    # G = 0: nothing to do, on both entries
    o, _ = enqueue_device(mt, sc, sc["kf_local"][None], G=0)
    torch.cuda.synchronize()
    for k in sent:
        assert S.same({k: o[k].cpu().numpy()}, {k: sent[k]}), k
    got = mt.local_ba(**S.call_args(sc, kf_local=np.zeros((0, F), np.uint8)))
    assert got["status"].shape == (0,) and got["pose"].shape == (0, F, 15)


def test_a_key_frame_table_longer_than_the_team(mt):
    """F = 517: the loops over the key frames take a second chunk of TEAM rows, the ranking of the free key frames carries its count from the first
    chunk into the second and adds the counts of the waves in front (free key frames in table rows 70, 300, 515 and 516; fixed ones in rows 5 and 513)"""
    sc = S.spread(S.make_scene(480, 4, 2, 50, setup=S.RGBD, noise=0.8, outliers=5, n_other=1), [70, 300, 515, 516, 5, 513, 130], TEAM + 5)
    assert dims(sc)[0] == TEAM + 5
    want = check(mt, sc)
    role = want["kf_role"][0]
    assert np.where(role == plp.LOCAL_BA_KF_FREE)[0].tolist() == [70, 300, 515, 516] and np.where(role == plp.LOCAL_BA_KF_FIXED)[0].tolist() == [5, 513]
    assert want["status"][0] == plp.LOCAL_BA_OK and (want["outlier"][0] == 1).any() and (want["pose"][0, 516] != -7.5).all() and (want["pose"][0, 514] == -7.5).all()


def test_more_free_key_frames_than_the_cap_is_a_status_with_nothing_else_written(mt):
    import torch
    sc = S.make_scene(470, 65, 1, 6, n_other=0)
    F, L, T = dims(sc)
    with pytest.raises(plp.PlpError) as e:
        host_model(sc, sc["kf_local"][None])
    assert e.value.status == plp.PLP_ERR_UNSUPPORTED
    o, _ = enqueue_device(mt, sc, sc["kf_local"][None])
    torch.cuda.synchronize()
    want = S.sentinel_out(1, F, L, T)
    want["status"][0] = plp.LOCAL_BA_TOO_MANY_FREE
    for k in want:
        assert S.same({k: o[k].cpu().numpy()}, {k: want[k]}), k
