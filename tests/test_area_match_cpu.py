"""area::match_in_consistent_area on the hand-built scenes of tests/area_match_scene.py, no GPU: the restatement (tests/area_match_ref.py) equals the
oracle exactly, the 64 x 48 scenes equal the reference build where it exists, every scene contains the case it is named for, and the scenes
together reach every reason and every fact of the census."""
import numpy as np
import pytest

import area_match_ref as R
import area_match_scene as S
import oracle_lib as O


def same(a, b):
    return a[2] == b[2] and a[0].dtype == b[0].dtype and np.array_equal(a[0], b[0]) and np.asarray(a[1], np.float32).tobytes() == np.asarray(b[1], np.float32).tobytes()


@pytest.mark.parametrize("check_orientation", (True, False))
@pytest.mark.parametrize("name", S.NAMES)
def test_restatement_equals_oracle(name, check_orientation):
    sc = S.scene(name)
    a = S.args(sc, check_orientation)
    want = O.match_area(*a)
    tie = O.angle_checker_last_tie()
    m, pp, num, census = R.match(*a)
    assert same((m, pp, num), want)
    if check_orientation:
        assert census["facts"]["bin_tie_at_cut"] == bool(tie)
    untouched = m < 0
    assert pp[untouched].tobytes() == sc["prev"][untouched].tobytes()
    if "kps3" in sc:                               # the second call of the initializer: frame 1 against frame 3 from the updated positions
        a3 = S.args(sc, check_orientation, frame=3, prev=want[1])
        assert same(R.match(*a3)[:3], O.match_area(*a3))


@pytest.mark.skipif(not O.ref2_path().exists(), reason="oracle/_ref/libplpref2.so not built (needs /root/reference)")
@pytest.mark.parametrize("check_orientation", (True, False))
@pytest.mark.parametrize("name", [n for n in S.NAMES if S.is_64x48(S.scene(n))])
def test_scene_equals_reference_build(name, check_orientation):
    sc = S.scene(name)
    frames = [(2, None)]
    want = O.match_area(*S.args(sc, check_orientation))
    if "kps3" in sc:
        frames.append((3, want[1]))
    for frame, prev in frames:
        a = S.args(sc, check_orientation, frame=frame, prev=prev)
        want = O.match_area(*a)
        with O.reference():
            got = O.match_area(*a)
        assert same(got, want), frame


@pytest.mark.parametrize("name", S.NAMES)
def test_scene_contains_its_case(name):
    sc = S.scene(name)
    m, pp, num, census = R.match(*S.args(sc, True))
    sc["check"](census, m, num)
    m_off, _, num_off, c_off = R.match(*S.args(sc, False))
    assert c_off["facts"]["orientation_removals"] == 0 and num_off == num + census["facts"]["orientation_removals"]
    assert np.array_equal(c_off["reason"], census["reason"])


def test_chained_call_needs_the_updated_points():
    sc = S.scene("chained")
    m1, pp1, n1, _ = R.match(*S.args(sc, True))
    assert pp1.tobytes() != sc["prev"].tobytes()
    m2, pp2, n2, c2 = R.match(*S.args(sc, True, frame=3, prev=pp1))
    assert n2 == 9 and (c2["reason"][3::4] == R.NO_CANDIDATE).all() and (m2[3::4] == -1).all()
    assert R.match(*S.args(sc, True, frame=3))[2] == 0            # from frame 1's own key points nothing of frame 3 is inside the margin
    assert pp2.tobytes() != pp1.tobytes()


def test_all_skipped_leaves_the_points():
    sc = S.scene("octaves_all_skipped")
    for check in (True, False):
        m, pp, num, _ = R.match(*S.args(sc, check))
        assert num == 0 and pp.tobytes() == sc["prev"].tobytes() and sc["prev"].tobytes() != np.stack([sc["kps1"]["x"], sc["kps1"]["y"]], 1).tobytes()


def test_census_reaches_every_reason_and_fact():
    reasons, facts = set(), {k: 0 for k in R.FACTS}
    for name in S.NAMES:
        c = R.match(*S.args(S.scene(name), True))[3]
        reasons |= set(c["reason"].tolist())
        for k in R.FACTS:
            facts[k] += int(c["facts"][k])
    assert reasons == set(range(len(R.REASONS)))
    assert all(v > 0 for v in facts.values()), facts


def test_the_ranking_of_equal_bins_decides_the_tie_scene():
    """the scene's tie is one a stable ranking and this machine's std::sort may settle differently; whichever bin survives, exactly one match goes"""
    sc = S.scene("orientation_tie")
    stable = lambda sizes: sorted(range(len(sizes)), key=lambda b: -sizes[b])
    m, _, num, c = R.match(*S.args(sc, True), rank_bins=stable)
    assert c["facts"]["bin_tie_at_cut"] and num == 6 and (m < 0).sum() == 1
