"""Scenes for the pose graph of DESIGN.md section 5, D22 (tests/test_pose_graph_cpu.py, tests/test_gpu_pose_graph.py, smoke): key frames on a ring with
accumulated drift, the graph tables of D21 built from an adjacency, and the per-problem mappings of a loop closure."""
import math

import numpy as np

import pose_optimizer_ref as D15
import transform_optimizer_ref as D16


def rot_z(a):
    c, s = math.cos(a), math.sin(a)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def rot_x(a):
    c, s = math.cos(a), math.sin(a)
    return np.array([[1.0, 0.0, 0.0], [0.0, c, -s], [0.0, s, c]])


def pose_row(R, t):
    return np.concatenate([R.reshape(-1), t, -R.T @ t])


def sim3_of(pose, scale=1.0):
    """g2o::Sim3(rot, trans, scale) of a pose row"""
    return np.array(D15.quat_from_rot([float(v) for v in pose[:9]]) + [float(pose[9]), float(pose[10]), float(pose[11]), float(scale)])


def ring_poses(F, rot_bias=0.004, trans_bias=0.02, tilt=0.3, turn=1.0):
    """(ground truth (F, 15), drifted (F, 15)): cameras on a circle (`turn` of it), each relative motion of the drifted track carries the same small error,
    so that the error grows along the track from row 0"""
    gt = []
    for i in range(F):
        a = 2.0 * math.pi * turn * i / F
        R_wc = rot_z(a) @ rot_x(tilt)
        c = np.array([5.0 * math.cos(a), 5.0 * math.sin(a), 0.3 * math.sin(3 * a)])
        gt.append((R_wc.T, -R_wc.T @ c))
    dr = [gt[0]]
    E = rot_z(rot_bias) @ rot_x(-0.5 * rot_bias)
    for i in range(1, F):
        R_rel = gt[i][0] @ gt[i - 1][0].T                     # T_i = T_rel T_{i-1}
        t_rel = gt[i][1] - R_rel @ gt[i - 1][1]
        R_rel, t_rel = E @ R_rel, (1.0 + trans_bias) * t_rel
        dr.append((R_rel @ dr[-1][0], R_rel @ dr[-1][1] + t_rel))
    return np.array([pose_row(R, t) for R, t in gt]), np.array([pose_row(R, t) for R, t in dr])


def graph_tables(F, pose, adj, parent, kf_id=None, erased=None, loops=None, slack=2):
    """D21's tables from adj {(i, j): weight} (taken both ways): kf_conn in ascending row, kf_covis in descending (weight, row); loops {row: [rows]}"""
    conn = [dict() for _ in range(F)]
    for (i, j), w in adj.items():
        conn[i][j] = w
        conn[j][i] = w
    cap = max([len(c) for c in conn] + [1]) + slack
    t = dict(pose=np.ascontiguousarray(pose, np.float64), kf_parent=np.asarray(parent, np.int32), kf_id=np.arange(F, dtype=np.int32) if kf_id is None else np.asarray(kf_id, np.int32),
             kf_erased=np.zeros(F, np.uint8) if erased is None else np.asarray(erased, np.uint8),
             kf_conn=np.full((F, cap), -1, np.int32), kf_conn_w=np.zeros((F, cap), np.int32), kf_n_conn=np.zeros(F, np.int32),
             kf_covis=np.full((F, cap), -1, np.int32), kf_covis_w=np.zeros((F, cap), np.int32), kf_n_covis=np.zeros(F, np.int32))
    for i, c in enumerate(conn):
        rows = sorted(c)
        t["kf_n_conn"][i] = t["kf_n_covis"][i] = len(rows)
        t["kf_conn"][i, :len(rows)] = rows
        t["kf_conn_w"][i, :len(rows)] = [c[r] for r in rows]
        order = sorted(rows, key=lambda r: (-c[r], -r))
        t["kf_covis"][i, :len(rows)] = order
        t["kf_covis_w"][i, :len(rows)] = [c[r] for r in order]
    off, flat = [0], []
    for i in range(F):
        flat += sorted((loops or {}).get(i, []))
        off.append(len(flat))
    t["kf_loop_offsets"], t["kf_loop"] = np.asarray(off, np.int32), np.asarray(flat, np.int32)
    return t


def band(F, extra, far_weight=50):
    """the adjacency of a chain with `extra` further strong edges (i, i - 2) for i = 2 .., then (i, i - 3), ...; one weak edge per row keeps every ordered
    list a proper prefix (the reference returns the EMPTY list when every entry reaches the weight)"""
    adj = {(i, i - 1): 150 for i in range(1, F)}
    left, d = extra, 2
    while left > 0 and d < F:
        for i in range(d, F):
            if left == 0:
                break
            adj[(i, i - d)] = 120
            left -= 1
        d += 1
    assert left == 0, "not that many pairs"
    for i in range(F):                                       # a weak partner that is no neighbour yet
        j = next((j for j in list(range(i + d + 1, F)) + list(range(i - d - 1, -1, -1)) if (i, j) not in adj and (j, i) not in adj), None)
        if j is not None:
            adj[(i, j)] = far_weight
    return adj


def ring(F, extra=0, fix_scale=False, loop_kf=0, arrow=False, turn=0.9, scale_drift=1.0, n_pre=2):
    """A loop closure over a ring of F key frames: the chain of parents, `extra` band edges, the current key frame F - 1 closes onto loop_kf.  The
    last n_pre key frames carry pre_corrected (ground truth, with scale_drift) and non_corrected (their drifted pose) Sim3; arrow: the key frame F - 1 also
    holds a loop edge to row 1, so that the last row block of the skyline starts at the first.  Returns (tables, [problem], ground truth (F, 15))."""
    gt, dr = ring_poses(F, turn=turn)
    adj = band(F, extra)
    loops = {F - 1: [1], 1: [F - 1]} if arrow and F > 3 else None
    t = graph_tables(F, dr, adj, [-1] + list(range(F - 1)), loops=loops)
    curr = F - 1
    pre = {r: sim3_of(gt[r], scale_drift) * np.array([1, 1, 1, 1, scale_drift, scale_drift, scale_drift, 1.0]) for r in range(max(F - n_pre, 1), F) if r != loop_kf}
    non = {r: sim3_of(dr[r]) for r in pre}
    pr = dict(loop_kf=loop_kf, curr_kf=curr, fix_scale=fix_scale, pre_corrected=pre, non_corrected=non, loop_connections={curr: {loop_kf}} if curr != loop_kf else {})
    return t, [pr], gt


def edge_count(F, extra, arrow=False):
    """the edges ring() makes: parents, the band, the loop connection (the arrow's loop edge is inserted once, from the later row)"""
    return (F - 1) + extra + (1 if F > 1 else 0) + (1 if arrow and F > 3 else 0)


def census():
    """16 key frames built to reach every rule of :131-298 (tests/test_pose_graph_cpu.py lists them): (tables, problems)"""
    F = 16
    gt, dr = ring_poses(F, turn=0.8)
    parent = [-1, 0, 1, 2, 3, 4, 5, 6, 7, 8, -1, 10, -1, 9, 13, 14]
    adj = {(i, i - 1): 150 for i in range(1, 10)}
    adj.update({(i, i - 2): 120 for i in range(2, 10)})
    adj.update({(0, 3): 40, (4, 8): 60, (2, 6): 30, (9, 4): 101, (7, 3): 110, (9, 2): 100, (8, 5): 105, (8, 3): 115})
    adj.update({(11, 10): 200, (13, 9): 160, (14, 13): 170, (15, 14): 150, (15, 13): 130, (15, 9): 20, (14, 9): 99, (15, 0): 10})
    kf_id = [2 * i for i in range(F)]
    kf_id[7] = 11                                            # below its parent's 12: key frame 7 adds nothing
    erased = np.zeros(F, np.uint8)
    erased[5] = 1
    loops = {8: [2, 3], 2: [8], 3: [8], 14: [1]}
    t = graph_tables(F, dr, adj, parent, kf_id=kf_id, erased=erased, loops=loops)
    assert t["kf_covis_w"][1, int(t["kf_n_covis"][1]) - 1] >= 100      # row 1 holds strong entries only: its covisibilities over weight come back empty
    pre = {15: sim3_of(gt[15], 1.05), 14: sim3_of(gt[14], 1.05)}
    non = {15: sim3_of(dr[15]), 14: sim3_of(dr[14])}
    lc = {15: {0, 9, 13}, 14: {0, 9}, 9: {4}, 5: {3}, 13: {14}}
    problems = [dict(loop_kf=0, curr_kf=15, fix_scale=False, pre_corrected=pre, non_corrected=non, loop_connections=lc),
                dict(loop_kf=3, curr_kf=15, fix_scale=True, pre_corrected={15: sim3_of(gt[15])}, non_corrected={15: sim3_of(dr[15])},
                     loop_connections={15: {3}, 9: {2}}),
                dict(loop_kf=5, curr_kf=15, fix_scale=False, pre_corrected={}, non_corrected={}, loop_connections={})]
    return t, problems


def landmarks(F, L, seed=3):
    """L landmarks with a reference row each: some erased, some with a reference that is outside the table: (pos_w, ref_kf, lm_erased)"""
    rng = np.random.default_rng(seed)
    pos = rng.uniform(-6.0, 6.0, (L, 3))
    ref = rng.integers(0, F, L).astype(np.int32)
    ref[::17] = F + 3
    ref[5::29] = -1
    er = (rng.uniform(size=L) < 0.1).astype(np.uint8)
    return pos, ref, er
