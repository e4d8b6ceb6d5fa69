"""CPU checks of the landmark normals and valid distance ranges (plp_landmark[_line]_geometry_*): the host build of
csrc/landmark_geometry.hpp (plp_model_landmark_geometry_host, the arithmetic the kernels run) against the restatement
tests/landmark_geometry_ref.py on the scene of tests/landmark_geometry_scene.py, bit for bit; hand cases of every rounding and of the two line
quirks; and that the scene can tell the reference's order of summation from any other.  The device is held to the same restatement in
tests/test_gpu_landmark_geometry.py."""
import math

import numpy as np
import pytest

import landmark_geometry_ref as G
import landmark_geometry_scene as S
import landmark_observe_ref as R
from plp import plp

f32 = np.float32


def model(sc, name, out=None, **over):
    t = {**sc[name], **over}
    lines = name == "lines"
    return plp.model_landmark_geometry(sc["pose"], t["feats"], t["pos_w"], t["ref_kf"], t["obs_offsets"], t["obs_kf"], t["obs_idx"], sc["scale_factors"],
                                       sc["scale_factors_lsd"] if lines else None, skip=t["skip"], counts=t["counts"], lines=lines, out=out)


@pytest.mark.parametrize("name", ["points", "lines"])
def test_model_equals_the_restatement_on_the_scene(name):
    sc = S.scene()
    want = S.want_points() if name == "points" else S.want_lines()
    got = model(sc, name, out=S.sentinels(sc[name]["L"], name == "lines"))
    st = want["status"]
    assert np.array_equal(got["status"], st)
    for k in want:                                              # values where UPDATED, the sentinels elsewhere: one comparison of all bytes
        assert S.same_bits(got[k], want[k]), k
    up = st == G.UPDATED
    assert (got["min_dist"][~up] == S.SENT_F32).all() and (got["max_dist"][~up] == S.SENT_F32).all()
    if name == "points":
        assert (got["normal"][~up] == S.SENT_F64).all()
        n = np.linalg.norm(got["normal"][up], axis=1)
        assert np.abs(n - 1).max() < 1e-15 and up.sum() > 500
    # the scene holds what its doc says: every status (points: all six; lines have no REF_NOT_OBSERVED), every special landmark
    assert set(st.tolist()) == ({0, 1, 2, 3, 4, 5} if name == "points" else {0, 1, 2, 4, 5})
    kinds = sc[name]["kinds"]
    expect = dict(all_keyframes=G.UPDATED, skipped=G.SKIPPED, skipped_without_observations=G.SKIPPED, ref_first=G.UPDATED, ref_last=G.UPDATED,
                  ref_missing=G.REF_NOT_OBSERVED if name == "points" else G.UPDATED, on_camera_centre=G.UPDATED, ref_kf_above_table=G.INDEX_RANGE,
                  ref_kf_negative=G.INDEX_RANGE, obs_kf_above_table=G.INDEX_RANGE, obs_kf_negative=G.INDEX_RANGE, feature_index_at_count=G.INDEX_RANGE,
                  feature_index_negative=G.INDEX_RANGE, octave_above_table=G.OCTAVE_RANGE, octave_negative=G.OCTAVE_RANGE)
    for l, kind in enumerate(kinds[:len(S.KINDS)]):
        assert st[l] == expect[kind], (kind, st[l])
    lens = np.diff(sc[name]["obs_offsets"])
    assert set(S.OBS_COUNTS) <= set(lens.tolist()) and lens.max() == S.F


def test_the_zero_term_of_a_landmark_on_a_camera_centre():
    sc = S.scene()
    t = sc["points"]
    l = t["kinds"].index("on_camera_centre")
    b, e = t["obs_offsets"][l], t["obs_offsets"][l + 1]
    terms = G.unit_terms([list(map(float, r)) for r in sc["pose"]], t["pos_w"][l], t["obs_kf"][b:e].tolist())
    assert terms[1] == (0.0, 0.0, 0.0) and all(abs(G.norm(*u) - 1) < 1e-15 for i, u in enumerate(terms) if i != 1)
    assert S.want_points()["status"][l] == G.UPDATED


def one_point(pos, centres, kfs, idxs, ref, octaves, sf, skip=None, counts=None, out=None):
    pose = np.zeros((len(centres), 15)); pose[:, 12:15] = centres
    kp = np.zeros((len(centres), len(octaves[0])), plp.KP_DTYPE); kp["octave"] = octaves
    return plp.model_landmark_geometry(pose, kp, [pos], [ref], [0, len(kfs)], kfs, idxs, sf, skip=skip, counts=counts, out=out)


def test_one_observation_gives_the_unit_vector_and_the_float_roundings():
    sf = R.scale_factors(1.2, 8)
    pos, c = (0.3, -1.7, 9.1), (1.25, 0.5, -0.75)
    d = [pos[i] - c[i] for i in range(3)]
    s = math.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
    for octave in range(8):
        got = one_point(pos, [c], [0], [2], 0, [[7, 7, octave, 7]], sf)
        assert got["status"][0] == G.UPDATED
        u = [d[i] / s for i in range(3)]
        assert got["normal"][0].tolist() == list(G.normalized(*u))      # the sum of one term, normalised once more (:293)
        mx = f32(s * float(sf[octave]))                                 # the f64 product, rounded once to float
        assert got["max_dist"][0] == mx and got["min_dist"][0] == f32(mx / sf[7])
    # the distance is one that tells the f64 product from the float product at some level
    assert any(f32(f32(s) * sf[o]) != f32(s * float(sf[o])) for o in range(8))


def test_point_statuses_by_hand_and_untouched_slots():
    sf = R.scale_factors(1.2, 8)
    cs = [(0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.0, 2.0, 0.0)]
    oc = [[0, 1, 2, 3]] * 3
    sent = lambda: dict(normal=np.full((1, 3), 9.0), min_dist=np.full(1, f32(9)), max_dist=np.full(1, f32(9)), status=np.full(1, 77, np.uint8))
    cases = [(dict(kfs=[0, 1], idxs=[1, 2], ref=1), G.UPDATED), (dict(kfs=[0, 1], idxs=[1, 2], ref=1, skip=[1]), G.SKIPPED),
             (dict(kfs=[], idxs=[], ref=1), G.NO_OBSERVATIONS), (dict(kfs=[0, 1], idxs=[1, 2], ref=2), G.REF_NOT_OBSERVED),
             (dict(kfs=[0, 1], idxs=[1, 2], ref=3), G.INDEX_RANGE), (dict(kfs=[0, 3], idxs=[1, 2], ref=0), G.INDEX_RANGE),
             (dict(kfs=[0, 1], idxs=[1, 4], ref=1), G.INDEX_RANGE), (dict(kfs=[0, 1], idxs=[1, 3], ref=1, counts=[4, 3, 4]), G.INDEX_RANGE),
             (dict(kfs=[0, 1], idxs=[1, 3], ref=1, octs=[[0, 1, 2, 8]] * 3), G.OCTAVE_RANGE)]
    for kw, want in cases:
        o = sent()
        got = one_point((0.5, 0.5, 4.0), cs, kw["kfs"], kw["idxs"], kw["ref"], kw.get("octs", oc), sf, skip=kw.get("skip"), counts=kw.get("counts"), out=o)
        assert got["status"][0] == want, (kw, got["status"])
        if want != G.UPDATED:
            assert (got["normal"] == 9.0).all() and got["min_dist"][0] == 9 and got["max_dist"][0] == 9, kw
        else:
            assert got["max_dist"][0] == f32(G.norm(-0.5, 0.5, 4.0) * float(sf[2]))


def one_line(pos, centres, kfs, idxs, ref, octaves, sf, sf_lsd, out=None):
    pose = np.zeros((len(centres), 15)); pose[:, 12:15] = centres
    kl = np.zeros((len(centres), len(octaves[0])), plp.KL_DTYPE); kl["octave"] = octaves
    return plp.model_landmark_geometry(pose, kl, [pos], [ref], [0, len(kfs)], kfs, idxs, sf, sf_lsd, lines=True, out=out)


def test_line_index_fallback_and_orb_table_divisor():
    sf, sf_lsd = R.scale_factors(1.2, 8), R.scale_factors(2.0, 2)
    pos = (0.5, 1.0, 6.0, 1.5, -1.0, 8.0)
    cs = [(0.0, 0.0, 0.0), (0.25, 0.5, -1.0)]
    d = G.norm(1.0 - 0.25, 0.0 - 0.5, 7.0 + 1.0)                       # the midpoint against the reference key frame's centre
    oc = [[0, 0, 0], [1, 0, 0]]                                         # key frame 1: level 1 at slot 0 only
    # the reference key frame is observed at slot 2 (level 0)
    got = one_line(pos, cs, [0, 1], [1, 2], 1, oc, sf, sf_lsd)
    assert got["status"][0] == G.UPDATED and got["max_dist"][0] == f32(d * 1.0)
    assert got["min_dist"][0] == f32(f32(d * 1.0) / sf[1])              # scale_factors_[nlevels - 1]: 1.2f of the ORB table, not 2.0f of the LSD table
    assert got["min_dist"][0] != f32(f32(d * 1.0) / sf_lsd[1])
    # the reference key frame is not among the observations: operator[] gives index 0, whose level is 1
    got = one_line(pos, cs, [0], [1], 1, oc, sf, sf_lsd)
    assert got["status"][0] == G.UPDATED and got["max_dist"][0] == f32(d * 2.0) and got["min_dist"][0] == f32(f32(d * 2.0) / sf[1])
    # num_levels_lsd above num_levels would index past scale_factors_: refused
    with pytest.raises(plp.PlpError):
        one_line(pos, cs, [0], [1], 1, oc, sf[:1], sf_lsd)


def test_bad_arguments_are_refused_by_the_model():
    sc = S.scene()
    t = sc["points"]
    with pytest.raises(plp.PlpError):
        model(sc, "points", obs_offsets=np.concatenate([[1], t["obs_offsets"][1:]]).astype(np.int32))
    bad = t["obs_offsets"].copy(); bad[5] = bad[6] + 1
    with pytest.raises(plp.PlpError):
        model(sc, "points", obs_offsets=bad)
    with pytest.raises(plp.PlpError):
        plp.model_landmark_geometry(sc["pose"], t["feats"], t["pos_w"], t["ref_kf"], t["obs_offsets"], t["obs_kf"], t["obs_idx"], np.ones(17, np.float32))
    assert plp.lib().plp_model_landmark_geometry_host(None, 0) == -1
    empty = plp.model_landmark_geometry(sc["pose"], t["feats"], np.zeros((0, 3)), [], [0], [], [], sc["scale_factors"])
    assert empty["status"].shape == (0,)


def test_the_scene_sees_a_wrong_order_of_summation():
    """The sum runs in list order, which is the reference's map order; the lists of the scene are in shuffled key-frame order, so a sum by ascending key
    frame, or a pairwise tree, must change the bits of mean_normal for at least half of the landmarks with 5 or more observations (a check of the
    INPUTS: with lists that were sorted, or too short, a kernel that reorders the sum would pass every comparison)."""
    sc = S.scene()
    t = sc["points"]
    want = S.want_points()
    lens = np.diff(t["obs_offsets"])
    up = want["status"] == G.UPDATED
    long_ = np.nonzero(up & (lens >= 5))[0]
    short = np.nonzero(up & (lens <= 2) & (lens > 0))[0]
    assert len(long_) >= 250 and len(short) >= 80
    # by ascending key frame
    srt = {k: v.copy() for k, v in t.items() if k in ("obs_kf", "obs_idx")}
    for l in range(t["L"]):
        b, e = t["obs_offsets"][l], t["obs_offsets"][l + 1]
        order = np.argsort(t["obs_kf"][b:e], kind="stable")
        srt["obs_kf"][b:e], srt["obs_idx"][b:e] = t["obs_kf"][b:e][order], t["obs_idx"][b:e][order]
    by_kf = G.refresh(sc["pose"], t["feats"]["octave"], t["counts"], sc["scale_factors"], t["pos_w"], t["ref_kf"], t["skip"], t["obs_offsets"], srt["obs_kf"],
                      srt["obs_idx"], out=S.sentinels(t["L"]))
    tree = S.restate(sc, "points", summation=G.sum_pairwise)
    for other, label in ((by_kf, "sorted by key frame"), (tree, "pairwise tree")):
        assert np.array_equal(other["status"], want["status"]), label
        assert S.same_bits(other["max_dist"], want["max_dist"]) and S.same_bits(other["min_dist"], want["min_dist"]), label   # the ranges have no sum in them
        differs = (other["normal"].view(np.uint64) != want["normal"].view(np.uint64)).any(axis=1)
        print(f"{label}: mean_normal changes for {int(differs[long_].sum())} of {len(long_)} landmarks with >= 5 observations")
        assert differs[long_].sum() * 2 >= len(long_), label
        assert not differs[short].any(), label                  # one or two terms: every order is the same sum
