"""Map culling and the covisibility graph (D21) against the REFERENCE'S OWN code: oracle/_ref/libplpref3.so is the
reference's data/graph_node.cc and module/local_map_cleaner.cc compiled UNMODIFIED by oracle/ref_build.sh against the stand-ins of
oracle/ref_shadow_map, driven through oracle/ref_driver3.cpp.  Three things are held equal, exactly (these modules are integers and bytes): the
reference build, the restatements (tests/covisibility_ref.py, tests/map_cull_ref.py) and the host build of csrc/covisibility.hpp and
csrc/map_cull.hpp (plp.model_*), which is the device's source.  The comparisons themselves are in tests/ref_map_lib.py, shared with
tests/test_oracle_golden_ref_map.py, which runs them on the committed answers where this library cannot be built.

Pinned by the reference's object code: everything in graph_node.cc -- update_connections, add_connection, erase_all_connections, the orders,
the queries --; the loops, the gates, the counting and the float decisions of local_map_cleaner.cc.  NOT pinned: the cascade of an erased key
frame (landmark::erase_observation, landmark::prepare_for_erasing, keyframe::erase_landmark_with_index), which the stand-ins restate from
landmark.cc and keyframe.cc: a second restatement, in C++, independent of tests/map_cull_ref.py.  The declared definitions stay definitions:
rows stand for pointers (the driver allocates a scene's key frames as one array), a row outside its table is no object -- a slot becomes
nullptr, an observation no entry, both counted -- and what the reference cannot be handed at all (a covisibility, a current key frame or a
fresh-list row outside its table) is left out of the comparison and counted: the counts are asserted below."""
import numpy as np
import pytest

import covisibility_scene as VS
import map_cull_scene as CS
import ref_map_lib as M

pytestmark = pytest.mark.skipif(not M.path().exists(), reason="oracle/_ref/libplpref3.so not built (needs the reference's sources)")

_ans = {}


def answers(kind, name=None):
    """the reference build's answers, computed once per scene"""
    if (kind, name) not in _ans:
        _ans[(kind, name)] = dict(covis=M.record_covis, cull=M.record_cull, lm=M.record_lm, chain=lambda _: M.record_chain())[kind](name)
    return _ans[(kind, name)]


@pytest.mark.parametrize("name", VS.SCENES)
def test_covisibility_equals_the_reference_build(name):
    """every owner list and every erase mask: C, O, the weights, the counts, parent and parent-unset, status, nearest and max_weight; the
    initial graph grown from `prev` by the reference's own update_connections(); the queries on the final graph; for f300 the chained
    sequence.  Nothing is left out: what the tables hold outside themselves became nullptr / no entry (hold_covis asserts the counts)"""
    assert M.hold_covis(answers("covis", name), name) > 60


# name -> (entries left out, problems left out).  mono65 and stereo97 run the lists of map_cull_scene._several: the two entries F + 3 and -1 of
# the fourth list and the fifth problem, whose current key frame is row F, cannot be handed to the reference.  4 of 96 and of 121 entries is
# above one in a hundred, which is why stereo97c -- stereo97's map and lists without them -- is there and leaves out nothing; every in-table
# entry and problem of the two scenes is compared all the same
LEFT_OUT = dict(mono97=(0, 0), mono65=(4, 1), stereo97=(4, 1), rgbd65=(0, 0), stereo97c=(0, 0), wrap65=(0, 0))


@pytest.mark.parametrize("name", CS.SCENES)
def test_keyframe_culling_equals_the_reference_build(name):
    """count_redundant_observations of every key frame (the reference's public function alone); per problem num_removed, the two masks and,
    per entry, the decision and the two counts derived from reference code by running every prefix of the list"""
    ans = answers("cull", name)
    n, out, problems, problems_out = M.hold_cull(ans, name)
    print(name, "entries compared", n, "left out", out, "problems compared", problems, "left out", problems_out)
    assert (out, problems_out) == LEFT_OUT[name]
    sc = CS.scene(name)
    slots, obs = ans[f"cull/{name}/dropped"][:2]
    print(name, "slots outside the table", int(slots), "of", sc["kf_lm"].size, "observations", int(obs), "of", len(sc["obs_kf"]))
    # rows that became nullptr / no entry: compared all the same, and few
    assert 100 * slots < sc["kf_lm"].size and 100 * obs < len(sc["obs_kf"])
    assert (slots > 0 and obs > 0) == (name == "stereo97")
    assert ans[f"cull/{name}/count/dropped"][:2].tolist() == [slots, obs]


def test_two_scenes_and_more_leave_nothing_out():
    assert sum(v == (0, 0) for v in LEFT_OUT.values()) >= 2 and set(LEFT_OUT) == set(CS.SCENES)


@pytest.mark.parametrize("name", list(CS.LM_SCENES))
def test_landmark_culling_equals_the_reference_build(name):
    """states, the compacted lists and num_removed; left out are the two rows L and -1 at the head of the last list: 2 of 628 entries"""
    n, out = M.hold_lm(answers("lm", name), name)
    print(name, "entries compared", n, "left out", out)
    assert out == 2 and 100 * out < n


def test_update_cull_update_chain_equals_the_reference_build():
    """the hand-over between D20 and D21 on one set of reference objects: remove_redundant_keyframes over the list the current key frame's own
    graph_node holds, prepare_for_erasing running the reference's erase_all_connections()"""
    M.hold_chain(answers("chain"))


def test_census_of_the_reference_run():
    """every quirk these modules must reproduce is reached by the reference run itself, read from its own outputs"""
    ans = {}
    for name in VS.SCENES:
        ans.update(answers("covis", name))
    for name in CS.SCENES:
        ans.update(answers("cull", name))
    for name in CS.LM_SCENES:
        ans.update(answers("lm", name))
    seen = M.census(ans, VS.SCENES)
    assert not [c for c in M.CENSUS if c not in seen]


def test_recording_twice_gives_the_same_answers():
    a, b = M.record_cull("wrap65"), M.record_covis("f5")
    for k, v in {**a, **b}.items():
        assert np.array_equal(v, {**answers("cull", "wrap65"), **answers("covis", "f5")}[k]), k
