"""GPU parity of k_quadtree's two paths: levels of at most kQtSmallN = 512 candidates (409 with the smaller LDS block of a per-level quota above 1960) are gathered by
element, sorted by rank and selected inside LDS; larger levels keep the radix sort over the HBM scratch (csrc/quadtree_kernel.hip).  Every case compares the per-level
quadtree output and the final key points with the oracle through the C ABI, and asserts the candidate counts it was built to hit.

Frames: isolated bright dots on a flat background.  A dot is one FAST candidate of level 0 (its whole ring is darker; no neighbour lies on the ring or touches it), so
the level-0 count is set on the host: dots are added from a fixed lattice until the ORACLE counts exactly the number wanted (CPU, deterministic)."""
import functools

import numpy as np
import pytest

import oracle_lib as O
from plp import plp

pytestmark = pytest.mark.gpu

SMALL_N, SMALL_N_SMALL_BLOCK = 512, 409      # qt_small_limit(2048), qt_small_limit(1024)
BG = 60


def lattice(h, w, step_x=8, step_y=8, rect=None, seed=0):
    """dot positions inside the FAST region (or inside rect = (x0, y0, x1, y1)), in a seeded random order"""
    x0, y0, x1, y1 = rect if rect else (24, 24, w - 24, h - 24)
    pts = [(x, y) for y in range(y0, y1, step_y) for x in range(x0, x1, step_x)]
    return [pts[i] for i in np.random.default_rng(seed).permutation(len(pts))]


def paint(h, w, pts, bright):
    img = np.full((h, w), BG, np.uint8)
    for (x, y), b in zip(pts, bright):
        img[y, x] = b
    return img


def level0_count(img, **kw):
    ora = O.OrbOracle(**kw)
    ora.extract(img)
    return len(ora.candidates(0))


@functools.lru_cache(maxsize=None)
def dot_frame(h, w, n0, equal=False, seed=0, K=1000, num_levels=8):
    """a frame whose level 0 has exactly n0 FAST candidates by the oracle's count"""
    pts = lattice(h, w, seed=seed)
    rng = np.random.default_rng(seed + 1)
    bright = np.full(len(pts), 200, np.uint8) if equal else rng.integers(120, 256, len(pts)).astype(np.uint8)
    k = n0
    for _ in range(8):     # one candidate per dot: the first guess is right unless a dot sits where a cell's tested block ends
        assert 0 <= k <= len(pts)
        img = paint(h, w, pts[:k], bright)
        got = level0_count(img, max_num_keypts=K, num_levels=num_levels)
        if got == n0:
            img.setflags(write=False)
            return img
        k += n0 - got
    raise AssertionError(f"no dot set with {n0} level-0 candidates")


def check(img, K=1000, want_n0=None, **kw):
    """one frame through the host entry point: candidates, per-level selection, key points and descriptors against the oracle; returns the per-level candidate counts"""
    ora = O.OrbOracle(K, **kw)
    ok, od = ora.extract(img)
    ex = plp.orb_extractor(K, **kw)
    gk, gd = ex.extract(img)
    counts = []
    for l in range(ex.get_num_scale_levels()):
        oc = ora.candidates(l)
        want = np.stack([oc["x"], oc["y"], oc["response"]], 1).astype(np.int32) if len(oc) else np.zeros((0, 3), np.int32)
        got = ex.debug_read(ex.DBG_CANDIDATES, l)
        assert np.array_equal(got, want), f"FAST candidates level {l}"
        counts.append(len(got))
        ol = ora.level_keypts(l)
        want = np.stack([ol["x"] - 19, ol["y"] - 19, ol["response"]], 1).astype(np.int32) if len(ol) else np.zeros((0, 3), np.int32)
        assert np.array_equal(ex.debug_read(ex.DBG_SELECTED, l), want), f"quadtree level {l} ({counts[-1]} candidates)"
    if want_n0 is not None:
        assert counts[0] == want_n0, counts
    assert np.array_equal(gk, ok) and np.array_equal(gd, od)
    return counts, gk


@pytest.mark.parametrize("n0", [SMALL_N - 1, SMALL_N, SMALL_N + 1])
def test_both_sides_of_the_small_path_limit(n0):
    """level 0 with 511 and 512 candidates (small path) and 513 (radix path); the quota of 217 makes the tree run both phases"""
    counts, gk = check(dot_frame(240, 320, n0), 1000, want_n0=n0)
    assert (gk["octave"] == 0).sum() >= 217


def test_all_scores_tie():
    """every dot equally bright: every node is decided by the smallest candidate index"""
    img = dot_frame(240, 320, 300, equal=True)
    ora = O.OrbOracle(1000)
    ora.extract(img)
    assert len(set(ora.candidates(0)["response"].tolist())) == 1
    check(img, 1000, want_n0=300)


def test_dense_rectangle_stalls_early():
    """480 dots, two pixels apart in x and four in y, inside ONE 96 x 40 rectangle around the centre: twice the quota, yet the reference's loop ends as soon as a pass
    leaves the list's length unchanged -- after the first split every node holds the dots in one corner and has a single child -- and keeps four key points"""
    h, w = 240, 320
    pts = lattice(h, w, 2, 4, rect=(100, 100, 196, 140), seed=3)
    img = paint(h, w, pts, np.random.default_rng(4).integers(120, 256, len(pts)).astype(np.uint8))
    counts, gk = check(img, 1000, want_n0=480)
    assert (gk["octave"] == 0).sum() == 4


def test_tight_clusters_deep_tree():
    """forty clusters of twelve dots (two pixels apart in x, four in y) spread over the frame: 480 candidates for a quota of 217, so phase 1 stops early, phase 2 splits
    the fullest nodes over several passes, and neighbours part only in the last splits before d_eff"""
    h, w = 240, 320
    pts = [(x0 + 2 * i, y0 + 4 * j) for y0 in range(30, 210, 38) for x0 in range(30, 290, 34) for j in range(3) for i in range(4)]
    img = paint(h, w, pts, np.random.default_rng(4).integers(120, 256, len(pts)).astype(np.uint8))
    counts, gk = check(img, 1000, want_n0=480)
    assert (gk["octave"] == 0).sum() >= 217


def test_fewer_candidates_than_the_quota():
    counts, gk = check(dot_frame(240, 320, 100, seed=5), 1000, want_n0=100)
    assert (gk["octave"] == 0).sum() == 100       # everything is kept


def test_levels_with_one_candidate_and_with_none():
    img = np.full((240, 320), BG, np.uint8)
    img[100, 100] = 200
    counts, _ = check(img, 1000, want_n0=1)
    assert counts.count(1) >= 2 and 0 in counts, counts        # the dot fades out of some levels of the pyramid
    counts, _ = check(np.full((240, 320), BG, np.uint8), 1000, want_n0=0)
    assert counts == [0] * 8


def test_batch_mixes_both_paths_and_an_empty_frame():
    """six frames in one launch: level 0 on the radix path (513 dots; noise: thousands of candidates on every level), on the small path (512, 300, 100 dots) and empty"""
    import torch
    h, w, K, cap = 240, 320, 1000, 2100
    noise = np.random.default_rng(9).integers(0, 256, (h, w), dtype=np.uint8)
    frames = np.stack([dot_frame(h, w, SMALL_N + 1), noise, dot_frame(h, w, 300, equal=True), np.full((h, w), BG, np.uint8), dot_frame(h, w, 100, seed=5),
                       dot_frame(h, w, SMALL_N)])
    want_n0 = [SMALL_N + 1, None, 300, 0, 100, SMALL_N]
    dev = torch.device("cuda:0")
    d = torch.from_numpy(frames).to(dev)
    ex = plp.orb_extractor(K)
    d_kps = torch.zeros((len(frames), cap, 28), dtype=torch.uint8, device=dev)
    d_desc = torch.zeros((len(frames), cap, 32), dtype=torch.uint8, device=dev)
    d_cnt = torch.zeros(len(frames), dtype=torch.int32, device=dev)
    ex.extract_batch(d, d_kps, d_desc, d_cnt)
    torch.cuda.synchronize()
    ex.last_batch_status()
    cnt = d_cnt.cpu().numpy()
    kps = d_kps.cpu().numpy().view(plp.KP_DTYPE).reshape(len(frames), cap)
    desc = d_desc.cpu().numpy()
    ora = O.OrbOracle(K)
    for f in range(len(frames)):
        ok, od = ora.extract(frames[f])
        n_cand = [len(ex.debug_read(ex.DBG_CANDIDATES, l, f)) for l in range(8)]
        assert n_cand == [len(ora.candidates(l)) for l in range(8)], f
        if want_n0[f] is not None:
            assert n_cand[0] == want_n0[f], (f, n_cand)
        else:
            assert min(n_cand[:4]) > SMALL_N, (f, n_cand)
        for l in range(8):
            ol = ora.level_keypts(l)
            want = np.stack([ol["x"] - 19, ol["y"] - 19, ol["response"]], 1).astype(np.int32) if len(ol) else np.zeros((0, 3), np.int32)
            assert np.array_equal(ex.debug_read(ex.DBG_SELECTED, l, f), want), (f, l, n_cand[l])
        assert cnt[f] == len(ok)
        assert np.array_equal(kps[f, :cnt[f]], ok) and np.array_equal(desc[f, :cnt[f]], od), f


@pytest.mark.parametrize("n0", [SMALL_N_SMALL_BLOCK, SMALL_N_SMALL_BLOCK + 1])
def test_small_path_with_the_smaller_lds_block(n0):
    """one level at K = 2000: the quota of 2000 halves the kernel's key block, which then holds the small path's arrays for 409 candidates and not for 410"""
    check(dot_frame(200, 280, n0, seed=7, K=2000, num_levels=1), 2000, want_n0=n0, num_levels=1)
