"""plp_match_area_host (k_match_area) against the oracle on the hand-built scenes of tests/area_match_scene.py: called through ctypes on buffers longer
than the call needs, filled with a sentinel.  What the call owns equals the oracle bit for bit, everything around it keeps the sentinel.
No tolerance anywhere: integers by equality, floats by bytes."""
import ctypes as C

import numpy as np
import pytest

import area_match_scene as S
import oracle_lib as O
from plp import plp

pytestmark = pytest.mark.gpu

PAD = 16                      # sentinel slots in front of and behind every output
I_SENT = np.int32(-1515870811)          # 0xA5A5A5A5
F_SENT = np.frombuffer(np.uint32(0xCDCDCDCD).tobytes(), np.float32)[0]


@pytest.fixture(scope="module")
def ctx():
    return plp.matcher()          # one context for the whole module: its scratch carries the stale contents of every earlier call


def grid_c(g6):
    return plp.match_grid_c(float(g6[0]), float(g6[1]), float(g6[2]), float(g6[3]), int(g6[4]), int(g6[5]))


def call(ctx, g, kps1, desc1, kps2, desc2, prev, margin, ratio, check_orientation, n1=None, n2=None):
    """-> (status, matched buffer, prev buffer, num buffer): each output with PAD sentinel slots on both sides of what the call may write"""
    k1 = np.ascontiguousarray(kps1, O.KP_DTYPE); k2 = np.ascontiguousarray(kps2, O.KP_DTYPE)
    d1 = np.ascontiguousarray(desc1, np.uint8); d2 = np.ascontiguousarray(desc2, np.uint8)
    n1 = len(k1) if n1 is None else n1
    n2 = len(k2) if n2 is None else n2
    matched = np.full(n1 + 2 * PAD, I_SENT, np.int32)
    pp = np.full(2 * n1 + 2 * PAD, F_SENT, np.float32)
    pp[PAD:PAD + 2 * n1] = np.asarray(prev, np.float32).reshape(-1)[:2 * n1]
    num = np.full(1 + 2 * PAD, I_SENT, np.int32)
    at = lambda a, off: C.c_void_p(a.ctypes.data + off * a.itemsize)
    st = plp.lib().plp_match_area_host(ctx._h, plp._p(k1), plp._p(d1), n1, plp._p(k2) if len(k2) else None, plp._p(d2) if len(k2) else None, n2, C.byref(g),
                                       at(pp, PAD), int(margin), float(ratio), int(check_orientation), at(matched, PAD), at(num, PAD))
    return st, matched, pp, num


def assert_equals(out, want, n1):
    st, matched, pp, num = out
    w_matched, w_pp, w_num = want
    assert st == plp.PLP_OK
    assert num[PAD] == w_num and np.array_equal(matched[PAD:PAD + n1], w_matched)
    assert pp[PAD:PAD + 2 * n1].tobytes() == np.asarray(w_pp, np.float32).tobytes()
    assert_padding(matched, pp, num, n1)


def assert_padding(matched, pp, num, n1):
    for a, n, s in ((matched, n1, I_SENT), (pp, 2 * n1, F_SENT), (num, 1, I_SENT)):
        side = np.concatenate([a[:PAD], a[PAD + n:]])
        assert side.tobytes() == np.full(2 * PAD, s, a.dtype).tobytes()


def run(ctx, sc, check, frame=2, prev=None):
    a = S.args(sc, check, frame=frame, prev=prev)
    return call(ctx, grid_c(a[0]), *a[1:])


@pytest.mark.parametrize("check_orientation", (True, False))
@pytest.mark.parametrize("name", S.NAMES)
def test_scene_equals_oracle(ctx, name, check_orientation):
    sc = S.scene(name)
    want = O.match_area(*S.args(sc, check_orientation))
    assert_equals(run(ctx, sc, check_orientation), want, len(sc["kps1"]))


@pytest.mark.parametrize("check_orientation", (True, False))
def test_chained_second_call_runs_on_the_first_calls_output(ctx, check_orientation):
    sc = S.scene("chained")
    n1 = len(sc["kps1"])
    first = run(ctx, sc, check_orientation)
    assert_equals(first, O.match_area(*S.args(sc, check_orientation)), n1)
    prev = first[2][PAD:PAD + 2 * n1].reshape(n1, 2).copy()
    assert prev.tobytes() != sc["prev"].tobytes()
    want = O.match_area(*S.args(sc, check_orientation, frame=3, prev=prev))
    assert want[2] == 9
    assert_equals(run(ctx, sc, check_orientation, frame=3, prev=prev), want, n1)


def test_scratch_regrown_then_reused_with_stale_contents():
    """n2 = 40, 5000, 40 on one fresh context: the scratch (matched distances and owners per key point of frame 2) grows for the second call, and
    the third runs in front of what the second left there"""
    own = plp.matcher()
    for n2, seed in ((40, 1), (5000, 2), (40, 3)):
        sc = S.lattice(70, n2, seed)
        want = O.match_area(*S.args(sc, True))
        assert want[2] >= 10
        assert_equals(run(own, sc, True), want, 70)


@pytest.mark.parametrize("name", ("steal_chain", "orientation_stolen"))
def test_python_entry_equals_oracle(name):
    sc = S.scene(name)
    for check in (True, False):
        want = O.match_area(*S.args(sc, check))
        got = plp.matcher(sc["ratio"], check).match_in_consistent_area(sc["kps1"], sc["desc1"], sc["kps2"], sc["desc2"], sc["prev"], sc["margin"], grid_c(sc["g6"]))
        assert got[2] == want[2] and np.array_equal(got[0], want[0]) and got[1].tobytes() == want[1].tobytes()


REFUSED_GRIDS = dict(cells_65537=(1, 65537), cells_257x256=(257, 256), cells_overflowing_int=(65536, 65536), no_columns=(0, 48), negative_rows=(64, -1))


@pytest.mark.parametrize("why", ("n2_65536",) + tuple(REFUSED_GRIDS))
def test_refusals_write_nothing(ctx, why):
    sc = S.scene("steal_chain")
    n1 = len(sc["kps1"])
    g = grid_c(sc["g6"])
    k2, d2, n2 = sc["kps2"], sc["desc2"], None
    if why == "n2_65536":
        k2 = np.zeros(65536, O.KP_DTYPE); d2 = np.zeros((65536, 32), np.uint8)
    else:
        g.cols, g.rows = REFUSED_GRIDS[why]
    st, matched, pp, num = call(ctx, g, sc["kps1"], sc["desc1"], k2, d2, sc["prev"], sc["margin"], sc["ratio"], True)
    assert st == plp.PLP_ERR_INVALID_ARG
    assert (matched == I_SENT).all() and (num == I_SENT).all()
    assert pp[PAD:PAD + 2 * n1].tobytes() == sc["prev"].tobytes()
    assert_padding(matched, pp, num, n1)


def test_empty_frame_1_counts_zero_and_writes_nothing_else(ctx):
    sc = S.scene("steal_chain")
    st, matched, pp, num = call(ctx, grid_c(sc["g6"]), sc["kps1"][:0], sc["desc1"][:0], sc["kps2"], sc["desc2"], sc["prev"][:0], sc["margin"], sc["ratio"], True)
    assert st == plp.PLP_OK and num[PAD] == 0
    assert_padding(matched, pp, num, 0)


def test_largest_accepted_grid_is_not_refused(ctx):
    """65536 cells is the most the key holds: the scene with the 256 x 256 grid runs (test_scene_equals_oracle), and so does a 65536 x 1 grid"""
    sc = S.scene("steal_chain")
    g6 = S.grid6(640, 480, 65536, 1)
    a = (g6,) + S.args(sc, True)[1:]
    assert_equals(call(ctx, grid_c(g6), *a[1:]), O.match_area(*a), len(sc["kps1"]))
