"""The stereo key-line problems above one workgroup of slots (256 left key lines) that tests/test_gpu_pair_kernels_wide.py runs on the
device and tests/test_pair_kernels_wide_cpu.py holds to their names on the restatement: _ragged_problem of
tests/test_gpu_stereo_keylines.py at two pairs of capacities, the left counts around one workgroup, and what the restatement
(tests/stereo_keylines_ref.py) makes of them."""
import functools

import numpy as np

import stereo_keylines_ref as SK
from test_gpu_stereo_keylines import EUROC, _ragged_problem, _random_pose

CAPS = [(257, 80), (600, 513)]                                  # (cap_left, cap_right): two and three workgroups of left key lines
B = 6
CAP_3D = 600


def left_counts(cap_l):
    return np.array((0, 255, 256, 257, cap_l, 1), np.int32)


@functools.lru_cache(maxsize=None)
def association(cap_l, cap_r):
    """S1 -> dict(kl_l, kl_r (B, cap) key lines, cl, cr counts, idx, dist (B, cap_l): the 1-NN, good / depths / x_right: per frame what the
    restatement returns for the slots below the left count).  Frames 3, 6, 2, 7, 1, 8 of a nine-frame _ragged_problem: the first has an
    empty right side, the full left side has a full right side, the others have what the generator drew; the left counts are
    left_counts(cap_l).  Planted where the left count is above 256 and the right side is not empty: left slot 256 and the last left slot
    have exact copies as partners (the last right slot and right slot 0), so they are kept whatever the generator drew."""
    rng = np.random.default_rng(900 + cap_l)
    kl_l, kl_r, _, cr, idx, dist = _ragged_problem(rng, 9, cap_l, cap_r)
    pick = [3, 6, 2, 7, 1, 8]
    kl_l, kl_r, cr, idx, dist = (np.ascontiguousarray(a[pick]) for a in (kl_l, kl_r, cr, idx, dist))
    cl = left_counts(cap_l)
    for b in range(B):
        if cl[b] > 256 and cr[b] > 1:
            for j, t in ((256, cr[b] - 1), (cl[b] - 1, 0)):
                kl_r[b][t] = kl_l[b][j]
                idx[b][idx[b] == t] = -1                        # nobody else names the planted partner
                idx[b][j], dist[b][j] = t, 20
    want = [SK.stereo_keylines(kl_l[b][:cl[b]], kl_r[b][:cr[b]], idx[b][:cl[b]], dist[b][:cl[b]]) for b in range(B)]
    return dict(kl_l=kl_l, kl_r=kl_r, cl=cl, cr=cr, idx=idx, dist=dist, good=[w[0] for w in want], depths=[w[1] for w in want],
                x_right=[w[2] for w in want])


@functools.lru_cache(maxsize=None)
def lines_3d(route):
    """S2 at cap CAP_3D -> dict(poses (B, 15), kl (B, cap), cl, pos_w / valid: per frame the restatement's, and the route's inputs): "stereo"
    takes good_match from S1's association, "rgbd" key-line depths of its own (some missing, some zero)"""
    a = association(*CAPS[1])
    assert a["kl_l"].shape[1] == CAP_3D
    rng = np.random.default_rng(950)
    poses = np.stack([_random_pose(rng) for _ in range(B)])
    kl, cl = a["kl_l"], a["cl"]
    if route == "stereo":
        good = np.stack([np.pad(a["good"][b], (0, CAP_3D - cl[b]), constant_values=-1) for b in range(B)]).astype(np.int32)
        want = [SK.keylines_3d(EUROC, SK.STEREO, poses[b], kl[b][:cl[b]], good_match=good[b][:cl[b]], kl_right=a["kl_r"][b][:a["cr"][b]])
                for b in range(B)]
        extra = dict(good_match=good, kl_r=a["kl_r"], cr=a["cr"])
    else:
        kd = rng.uniform(0.5, 8.0, (B, CAP_3D, 2)).astype(np.float32)
        kd[rng.random((B, CAP_3D)) < 0.08] = -1.0               # compute_stereo_from_depth's "no depth" ...
        kd[rng.random((B, CAP_3D, 2)) < 0.04] = 0.0             # ... and a zero depth at one end
        want = [SK.keylines_3d(EUROC, SK.RGBD, poses[b], kl[b][:cl[b]], kl_depths=kd[b][:cl[b]]) for b in range(B)]
        extra = dict(kl_depths=kd)
    return dict(poses=poses, kl=kl, cl=cl, pos_w=[w[0] for w in want], valid=[w[1] for w in want], **extra)
