"""Plain-Python restatement of DESIGN.md section 5, D23: optimize::global_bundle_adjuster::optimize over the point map and the array half of
module::loop_bundle_adjuster's map update.  D23 is written on top of D17 and D15 and restates only what differs; what it takes from them unchanged
(the edges, the sums, the Schur solve, the Cholesky, Levenberg-Marquardt) is tests/local_ba_ref.py's Problem and tests/pose_optimizer_ref.py.  Python
floats only.  The host build of csrc/global_ba.hpp is held to this bit for bit (tests/test_global_ba_cpu.py)."""
import local_ba_ref as R17
import pose_optimizer_ref as R15

OK, NO_EDGES, STOPPED = 0, 1, 2
KF_NOT_REACHED, KF_OPTIMIZED, KF_PROPAGATED, KF_ERASED = 0, 1, 2, 3
LM_NO_REF, LM_OPTIMIZED, LM_MOVED, LM_ERASED = 0, 1, 2, 3
SENTINEL = dict(status=0xEE, kf_optimized=0x77, lm_optimized=0x77, pose=-7.25, pos_w=-7.25, info=-33, chi2=-7.25)
PROP_SENTINEL = dict(pose=-7.25, pose_before=-7.25, kf_status=0xEE, pos_w=-7.25, lm_status=0xEE)


def cam_center(p):
    return [((-p[i]) * p[9] + (-p[3 + i]) * p[10]) + (-p[6 + i]) * p[11] for i in range(3)]


class Problem(R17.Problem):
    """D17's problem; the damped solves are counted (out_info[2]: one factorisation per try)"""
    tries = 0

    def solve(self, Hpp, Hll, W, lam):
        self.tries += 1
        return super().solve(Hpp, Hll, W, lam)


def optimize(Tb, num_iter=10, use_huber_kernel=True, stop=False):
    """one run: dict(status, kf_optimized [F], lm_optimized [L], pose {f: 15}, pos_w {l: 3}, info [4], chi2 [3], problem)"""
    if stop:
        return dict(status=STOPPED)
    # the sets: every key frame that is not erased is a vertex (D17's sets with every key frame marked local: no key frame is left to be fixed)
    P = Problem(Tb, [1] * Tb.F)
    out = dict(kf_optimized=[int(not e) for e in Tb.kf_erased], info=[0, 0, 0, 0], chi2=[0.0, 0.0, 0.0], problem=P)
    vertices = [f for f in range(Tb.F) if not Tb.kf_erased[f]]
    if not P.edges:
        out.update(status=NO_EDGES, lm_optimized=[0] * Tb.L, pos_w={})
        out["pose"] = {f: [float(v) for v in Tb.pose[f][:12]] + cam_center([float(v) for v in Tb.pose[f][:12]]) for f in vertices}
        return out
    P.current, P.lam, P.ni = 0.0, 0.0, 2.0
    P.round_setup()                                          # no level: every edge is live
    its, rej, end, cur, lam = P.optimize(num_iter, bool(use_huber_kernel))
    out["status"] = OK
    out["lm_optimized"] = [int(l in P.by_lm) for l in range(Tb.L)]
    out["pose"] = {f: R15.pose_from_est(P.kf_est[f]) for f in vertices}       # the origin and a key frame without an edge: the converted input
    out["pos_w"] = {l: list(P.lm_est[l]) for l in P.la}
    out["info"] = [its, rej, P.tries, end if end else (R15.END_ITERATIONS if its else 0)]
    out["chi2"] = [P.start_chi[0], P.current, P.lam]
    return out


# ---- the loop adjuster's map update
def mul(a, b):
    """c = a * b of affine 3 x 4 maps (9 rotation entries row-major, 3 translation): three-term sums left to right, translation (R_a t_b) + t_a"""
    c = [0.0] * 12
    for i in range(3):
        for j in range(3):
            c[3 * i + j] = (a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j]) + a[3 * i + 2] * b[6 + j]
        c[9 + i] = ((a[3 * i] * b[9] + a[3 * i + 1] * b[10]) + a[3 * i + 2] * b[11]) + a[9 + i]
    return c


def inv(p):
    """pose_inv as set_cam_pose stores it: rot^T and -rot^T t"""
    return [p[3 * j + i] for i in range(3) for j in range(3)] + cam_center(p)


def propagate(pose, kf_parent, kf_optimized, pose_after, pos_w, ref_kf, lm_optimized, pos_after, kf_erased=None, kf_is_origin=None, lm_erased=None):
    """the queue walk of module/loop_bundle_adjuster.cc:110-143 over children lists, then :146-181: dict(pose {f: 15}, pose_before {f: 12}, kf_status [F],
    pos_w {l: 3}, lm_status [L])"""
    F, L = len(pose), len(pos_w)
    kf_erased = kf_erased if kf_erased is not None else [0] * F
    kf_is_origin = kf_is_origin if kf_is_origin is not None else [0] * F
    lm_erased = lm_erased if lm_erased is not None else [0] * L
    children = [[] for _ in range(F)]
    for c in range(F):
        p = int(kf_parent[c])
        if not kf_erased[c] and not kf_is_origin[c] and 0 <= p < F and not kf_erased[p]:
            children[p].append(c)
    status = [KF_ERASED if kf_erased[f] else KF_NOT_REACHED for f in range(F)]
    after = {}
    queue = [f for f in range(F) if kf_is_origin[f] and not kf_erased[f]]
    for f in queue:
        if kf_optimized[f]:
            after[f] = [float(v) for v in pose_after[f][:12]]
    seen = set(queue)
    while queue:
        parent = queue.pop(0)
        pose_wp = inv([float(v) for v in pose[parent][:12]])
        for child in children[parent]:
            if child in seen:                                # a table that is no tree: every key frame is walked once
                continue
            seen.add(child)
            if kf_optimized[child]:
                after[child] = [float(v) for v in pose_after[child][:12]]
            elif parent in after:
                pose_cp = mul([float(v) for v in pose[child][:12]], pose_wp)
                after[child] = mul(pose_cp, after[parent])
            queue.append(child)
        if parent in after:
            status[parent] = KF_OPTIMIZED if kf_optimized[parent] else KF_PROPAGATED
    out = dict(kf_status=status, pose={f: after[f] + cam_center(after[f]) for f in after}, pose_before={f: [float(v) for v in pose[f][:12]] for f in after},
               pos_w={}, lm_status=[0] * L)
    for l in range(L):
        if lm_erased[l]:
            out["lm_status"][l] = LM_ERASED
        elif lm_optimized[l]:
            out["pos_w"][l] = [float(v) for v in pos_after[l]]
            out["lm_status"][l] = LM_OPTIMIZED
        else:
            r = int(ref_kf[l])
            if not (0 <= r < F) or r not in after:
                out["lm_status"][l] = LM_NO_REF
                continue
            b = [float(v) for v in pose[r][:12]]
            p = [float(v) for v in pos_w[l]]
            pc = [((b[3 * i] * p[0] + b[3 * i + 1] * p[1]) + b[3 * i + 2] * p[2]) + b[9 + i] for i in range(3)]
            wc = inv(after[r])
            out["pos_w"][l] = [((wc[3 * i] * pc[0] + wc[3 * i + 1] * pc[1]) + wc[3 * i + 2] * pc[2]) + wc[9 + i] for i in range(3)]
            out["lm_status"][l] = LM_MOVED
    return out
