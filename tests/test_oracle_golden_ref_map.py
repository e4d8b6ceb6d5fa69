"""The restatements (tests/covisibility_ref.py, tests/map_cull_ref.py) and the host build of csrc/covisibility.hpp and csrc/map_cull.hpp
against the committed answers of the REFERENCE BUILD (tests/golden/ref_map.npz, written by tools/make_golden_ref.py from
oracle/_ref/libplpref3.so = the reference's data/graph_node.cc and module/local_map_cleaner.cc, compiled unmodified): the comparisons of
tests/test_oracle_vs_ref_map.py without the library, so this check travels; tests/test_gpu_golden_ref_map.py holds the device entries to the
same file.  The file stores answers only; the scenes are regenerated from their seeds and a digest of every scene's input tables is asserted
first, so a drifted scene fails there and is not compared with stale answers.  f1100 is not in the file (its tables would not fit).

From the reference's object code: everything of graph_node.cc; the loops, gates, counts and float decisions of local_map_cleaner.cc.  From the
stand-ins of oracle/ref_shadow_map (a second restatement, not a pin): the cascade of an erased key frame."""
import numpy as np
import pytest

import map_cull_scene as CS
import ref_map_lib as M
from test_oracle_vs_ref_map import LEFT_OUT


@pytest.fixture(scope="module")
def ans():
    return M.load_golden()


@pytest.mark.parametrize("name", M.GOLDEN_COVIS)
def test_covisibility_equals_the_committed_reference_answers(ans, name):
    assert M.hold_covis(ans, name) > 60


@pytest.mark.parametrize("name", CS.SCENES)
def test_keyframe_culling_equals_the_committed_reference_answers(ans, name):
    n, out, problems, problems_out = M.hold_cull(ans, name)
    assert (out, problems_out) == LEFT_OUT[name] and n >= 25


@pytest.mark.parametrize("name", list(CS.LM_SCENES))
def test_landmark_culling_equals_the_committed_reference_answers(ans, name):
    n, out = M.hold_lm(ans, name)
    assert out == 2 and 100 * out < n


def test_chain_equals_the_committed_reference_answers(ans):
    M.hold_chain(ans)


def test_census_of_the_committed_answers(ans):
    """the quirks are reached by the recorded reference run too, without f1100"""
    seen = M.census(ans)
    assert not [c for c in M.CENSUS if c not in seen]


def test_a_drifted_scene_fails_at_its_digest(ans):
    bad = dict(ans)
    bad["cull/wrap65/digest"] = np.roll(ans["cull/wrap65/digest"], 1)
    with pytest.raises(AssertionError, match="not the ones the answers were recorded from"):
        M.hold_cull(bad, "wrap65")
