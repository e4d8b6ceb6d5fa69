"""CPU-only: the path a matcher call takes (plp_match_debug_plan, the same host function launch_match launches from), pinned on both
sides of every boundary: the brute-force LDS staging, the windowed LDS staging with and without t_x_right (reached through n_cap and
through t_count_hint), the 255-cell grid limit of k_match_prep, B = 64 and n_cap = 512.  tests/test_gpu_match_paths.py runs each path."""
import pytest

from plp import plp

P = plp
G64 = plp.make_grid(640, 480)                       # 64 x 48


def grid(cols, rows):
    return plp.make_grid(640, 480, cols, rows)


def plan(mode, B=1, n_cap=1000, m_cap=1000, g=G64, xr=False, hint=0):
    return plp.match_plan(mode, B, n_cap, m_cap, grid=g, t_x_right=xr, t_count_hint=hint)


CELLS_1 = ("cells", "grid", 32, "sorted")
CELLS_64 = ("cells", "grid", 512, "sorted")
LDS = ("lds", "point", 128, "generic")
TOPK_POINT = ("topk", "point", 0, "generic")
LANES_POINT = ("lanes", "point", 0, "generic")


def test_brute_force_lds_staging_ends_at_2048_targets():
    for B in (1, 63, 64, 200):
        assert plan(P.MODE_BRUTE_FORCE, B, 2048) == LDS
        assert plan(P.MODE_BRUTE_FORCE, B, 2049) == TOPK_POINT
        assert plan(P.MODE_BRUTE_FORCE, B, 4000) == TOPK_POINT
        assert plan(P.MODE_BRUTE_FORCE, B, 512) == LDS          # small target sets in large batches stay in LDS, never one lane per query
        assert plan(P.MODE_BRUTE_FORCE, B, 8192) == TOPK_POINT


@pytest.mark.parametrize("mode", [P.MODE_LANDMARKS, P.MODE_LAST_FRAME])
def test_windowed_lds_staging(mode):
    # 16 (12) bytes per staged target + 2 x 4104 cell starts <= 64 KB
    assert plan(mode, 1, 3583, xr=True) == CELLS_1
    assert plan(mode, 1, 3584, xr=True) == TOPK_POINT
    assert plan(mode, 1, 4777, xr=False) == CELLS_1
    assert plan(mode, 1, 4778, xr=False) == TOPK_POINT
    assert plan(mode, 1, 3584, xr=False) == CELLS_1
    # the same boundaries reached through the hint on a large capacity; a hint above n_cap counts as n_cap
    assert plan(mode, 1, 8192, xr=True, hint=3583) == CELLS_1
    assert plan(mode, 1, 8192, xr=True, hint=3584) == TOPK_POINT
    assert plan(mode, 1, 8192, xr=False, hint=4777) == CELLS_1
    assert plan(mode, 1, 8192, xr=False, hint=4778) == TOPK_POINT
    assert plan(mode, 1, 3583, xr=True, hint=9000) == CELLS_1
    assert plan(mode, 1, 3584, xr=True, hint=9000) == TOPK_POINT
    assert plan(mode, 70, 8192, xr=True, hint=3583) == CELLS_64


@pytest.mark.parametrize("mode", [P.MODE_LANDMARKS, P.MODE_LAST_FRAME])
def test_windowed_grid_limit_of_the_cells_path(mode):
    assert plan(mode, 1, 1000, g=grid(255, 16)) == CELLS_1
    assert plan(mode, 1, 1000, g=grid(256, 16)) == TOPK_POINT
    assert plan(mode, 1, 1000, g=grid(16, 255)) == CELLS_1
    assert plan(mode, 1, 1000, g=grid(16, 256)) == TOPK_POINT
    assert plan(mode, 1, 1000, g=grid(4096, 1)) == TOPK_POINT
    # beyond the cells path: one lane per query for <= 512 targets in >= 64 problems, else one wave per query
    assert plan(mode, 64, 512, g=grid(256, 16)) == LANES_POINT
    assert plan(mode, 64, 513, g=grid(256, 16)) == TOPK_POINT
    assert plan(mode, 63, 512, g=grid(256, 16)) == TOPK_POINT
    assert plan(mode, 64, 512, g=grid(16, 256)) == LANES_POINT
    assert plan(mode, 64, 512, g=grid(255, 16)) == CELLS_64


@pytest.mark.parametrize("mode", [P.MODE_LANDMARKS, P.MODE_LAST_FRAME])
def test_windowed_queries_per_workgroup_follow_the_batch(mode):
    assert plan(mode, 63) == CELLS_1
    assert plan(mode, 64) == CELLS_64
    assert plan(mode, 1, 1) == CELLS_1


@pytest.mark.parametrize("mode,fam", [(P.MODE_LANDMARKS_LINE, "line"), (P.MODE_LAST_FRAME_LINE, "line"), (P.MODE_BOW, "group"),
                                      (P.MODE_TRIANGULATION, "group")])
def test_generic_modes_lanes_or_topk(mode, fam):
    lanes, topk = ("lanes", fam, 0, "generic"), ("topk", fam, 0, "generic")
    assert plan(mode, 64, 512) == lanes
    assert plan(mode, 64, 513) == topk
    assert plan(mode, 63, 512) == topk
    assert plan(mode, 500, 1) == lanes
    assert plan(mode, 1, 1) == topk
    assert plan(mode, 64, 512, xr=True, hint=100, g=grid(1, 1)) == lanes      # the windowed-mode inputs do not move these modes
    assert plan(mode, 1, 8192) == topk


@pytest.mark.parametrize("mode", [P.MODE_FUSE, P.MODE_FUSE_LINE])
def test_fuse_modes(mode):
    for B, n in ((1, 1), (64, 512), (70, 8192)):
        assert plan(mode, B, n) == ("fuse", "any", 0, None)


def test_every_mode_has_a_family_and_an_empty_side_runs_nothing():
    fams = {P.MODE_LANDMARKS: "grid", P.MODE_LAST_FRAME: "grid", P.MODE_BRUTE_FORCE: "point", P.MODE_LANDMARKS_LINE: "line",
            P.MODE_LAST_FRAME_LINE: "line", P.MODE_BOW: "group", P.MODE_FUSE: "any", P.MODE_FUSE_LINE: "any", P.MODE_TRIANGULATION: "group"}
    assert sorted(fams) == list(range(9))
    for mode, fam in fams.items():
        assert plan(mode)[1] == fam
        assert plan(mode, 3, 0, 10) == (None, "any", 0, None)
        assert plan(mode, 3, 10, 0) == (None, "any", 0, None)
    for bad in (dict(mode=9), dict(mode=-1), dict(B=0), dict(n_cap=8193), dict(n_cap=-1)):
        kw = dict(mode=P.MODE_LANDMARKS, B=1, n_cap=10, m_cap=10, g=G64)
        kw.update(bad)
        with pytest.raises(plp.PlpError):
            plan(**kw)
