"""Restatement of DESIGN.md section 5, D26 in plain Python: Planar_Mapping_module::refinement() (planar_mapping_module.cc:773-793), merge_planes
(:795-898), refine_planes (:900-952), refine_points (:954-1004) and Plane::merge (data/landmark_plane.cc:221-248) with the reference's loops as
written, over objects: a plane holds its landmarks as a dict keyed by landmark (an unordered_map keyed by id_, iterated in insertion = slot order:
D19 item 1), a landmark its owner.  Written from the reference's text and D26, not from csrc/plane_refinement.hpp.  The arithmetic of an update and
of a moved point is plane_ransac_ref's.  `census` collects which branches a run took."""
import numpy as np

import plane_ransac_ref as PR

IN_DB, VALID, NEED = 1, 2, 4
STAGE_MERGE, STAGE_PLANES, STAGE_POINTS, STAGE_ALL = 1, 2, 4, 7
OK, TOO_FEW_PLANES, OVERFLOW = range(3)
NO_UPDATE = 255
SENTINEL = dict(status=0xEE, was_merged=0xEE, planes_changed=0xEE, points_changed=0xEE, removed=0xEE, num_merges=-77, merges=-77, num_updates=-77,
                update_status=0xEE, lm_changed=0xEE)
DTYPES = dict(status=np.uint8, was_merged=np.uint8, planes_changed=np.uint8, points_changed=np.uint8, removed=np.uint8, num_merges=np.int32,
              merges=np.int32, num_updates=np.int32, update_status=np.uint8, lm_changed=np.uint8)
TABLE_DTYPES = dict(pl_state=np.uint8, pl_equation=np.float64, pl_best_error=np.float64, pl_count=np.int32, pl_lm=np.int32, pos_w=np.float64,
                    lm_erased=np.uint8, lm_owner=np.int32)


class Overflow(Exception):
    pass


class Plane:
    def __init__(self, row, state, eq, best_error, slots, count):
        self.row = row
        self.in_db, self.valid, self.need = bool(state & IN_DB), bool(state & VALID), bool(state & NEED)
        self.other_bits = int(state) & ~7
        self.eq = [float(x) for x in eq]
        self.best_error = float(best_error)
        self.slots = [int(x) for x in slots]                      # the row of pl_lm as the library keeps it
        self.lms = {lm: lm for lm in self.slots[:count]}          # _landmarks

    def state(self):
        return self.other_bits | (IN_DB if self.in_db else 0) | (VALID if self.valid else 0) | (NEED if self.need else 0)

    def abs_n(self):
        with np.errstate(all="ignore"):
            a, b, c = (np.float64(x) for x in self.eq[:3])
            return np.sqrt((a * a + b * b) + c * c)


class Map:
    """one problem: the planes by row, the landmark tables, the settings"""

    def __init__(self, t, g, dist_thresh, error_thresh, points_per_ransac, iters, dot_product_threshold, offset_delta_factor, seed):
        NP, self.n_cap = t["pl_lm"].shape[1], t["pl_lm"].shape[2]
        self.planes = [Plane(r, t["pl_state"][g, r], t["pl_equation"][g, r], t["pl_best_error"][g, r], t["pl_lm"][g, r],
                             min(max(int(t["pl_count"][g, r]), 0), self.n_cap)) for r in range(NP)]
        self.pos = np.array(t["pos_w"][g], np.float64)
        self.erased = [bool(x) for x in t["lm_erased"][g]]
        self.owner = [int(x) for x in t["lm_owner"][g]]           # a row, -1 = nullptr
        self.L = len(self.owner)
        self.dist_thresh, self.error_thresh = float(dist_thresh), float(error_thresh)
        self.ppr, self.iters, self.dot_thr, self.factor, self.seed = int(points_per_ransac), int(iters), float(dot_product_threshold), int(offset_delta_factor), int(seed) + g
        self.calls = 0                                            # update calls so far
        self.update_status = {}
        self.merges, self.removed = [], {}
        self.lm_changed = np.zeros(self.L, np.uint8)
        self.census = set()
        listed = [lm for p in self.planes if p.in_db for lm in p.lms]
        if len(listed) != len(set(listed)):
            self.census.add("lm_in_two_lists")

    # -- landmarks
    def named(self, lm):
        return 0 <= lm < self.L

    def will_be_erased(self, lm):
        return not self.named(lm) or self.erased[lm]

    def all_planes(self):
        """get_all_landmark_planes(): by definition the rows in the database, ascending"""
        return [p for p in self.planes if p.in_db]

    def remove_landmarks_ownership(self, plane, where):           # landmark_plane.cc:197-207
        for lm in plane.lms:
            if self.named(lm):
                if self.owner[lm] not in (-1, plane.row):
                    self.census.add(where + "_clears_foreign_owner")
                self.owner[lm] = -1

    # -- Plane::merge (landmark_plane.cc:221-248)
    def merge(self, this, other):
        landmarks = dict(other.lms)
        fresh = [lm for lm in landmarks if not self.will_be_erased(lm) and lm not in this.lms]
        if len(this.lms) + len(fresh) > self.n_cap:
            self.census.add("overflow")
            raise Overflow()
        self.remove_landmarks_ownership(other, "merge")
        for lm in landmarks:
            if self.will_be_erased(lm):
                self.census.add("merge_erased_member")
                continue
            if lm in this.lms:
                self.census.add("entry_already_present")
            else:
                this.slots[len(this.lms)] = lm
            this.lms[lm] = lm
            self.owner[lm] = this.row
        this.need = True
        other.valid = False

    # -- update_plane_via_RANSAC (:593-733): D19's UPDATE on the row's current list
    def update_plane_via_RANSAC(self, plane):
        c, self.calls = self.calls, self.calls + 1
        lms = list(plane.lms)
        pos = np.array([self.pos[lm] if self.named(lm) else [0.0, 0.0, 0.0] for lm in lms], np.float64).reshape(-1, 3)
        flags = np.array([PR.LM_ERASED if self.will_be_erased(lm) else (PR.LM_OWNED if self.owner[lm] >= 0 else 0) for lm in lms], np.uint8)
        if np.any(flags & PR.LM_ERASED):
            self.census.add("update_erased_member")
        r = PR.ransac(PR.UPDATE, pos, flags, self.dist_thresh, self.error_thresh, points_per_ransac=self.ppr, iters=self.iters,
                      best_error_in=plane.best_error, equation_in=plane.eq, seed=self.seed, p=c)
        self.update_status[plane.row] = r["status"]
        self.census.add(f"update_status_{r['status']}")
        plane.eq, plane.best_error = [float(x) for x in r["equation"]], float(r["best_error"])
        if r["flags"] & PR.FLAG_INVALID:
            plane.valid = False
        if r["flags"] & PR.FLAG_NEED_REFINEMENT:
            plane.need = True
        if r["status"] != PR.OK:
            return False
        self.remove_landmarks_ownership(plane, "update")                  # :728
        kept = [lms[s] for s in range(len(lms)) if r["inliers"][s]]
        plane.lms = {lm: lm for lm in kept}                       # :729
        plane.slots[:len(kept)] = kept
        for lm in kept:                                           # :730
            self.owner[lm] = plane.row
        return True

    # -- merge_planes (:795-898)
    def merge_planes(self):
        all_planes = self.all_planes()
        if len(all_planes) < 2:                                   # :799-808
            return False
        with np.errstate(all="ignore"):
            offset_thr = np.float64(self.factor) * np.float64(self.dist_thresh)          # :813
        planes_will_be_removed = []
        was_merged = False
        for i in range(len(all_planes)):
            if not all_planes[i].valid:                           # :820
                continue
            parent_merged = False
            j = i + 1
            while j < len(all_planes):
                if not all_planes[j].valid:                       # :828-835
                    self.census.add("skip_invalid")
                    j += 1
                    if j >= len(all_planes):
                        self.census.add("skip_break")
                        break
                    if not all_planes[j].valid:
                        self.census.add("skip_then_tested_invalid")
                pi, pj = all_planes[i], all_planes[j]
                with np.errstate(all="ignore"):
                    ni, nj = np.float64(1.0) / pi.abs_n(), np.float64(1.0) / pj.abs_n()
                    offset_delta = np.float64(pi.eq[3]) * ni - np.float64(pj.eq[3]) * nj
                    a, b = [np.float64(x) for x in pi.eq[:3]], [np.float64(x) for x in pj.eq[:3]]
                    dot = ((a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]) * (ni * nj)
                    ao, ad = abs(offset_delta), abs(dot)
                if ao > offset_thr and ad < self.dot_thr:         # :853
                    self.census.add("pair_far_offset_and_angle")
                elif ao < offset_thr and ad > self.dot_thr:       # :859
                    self.census.add("pair_merge")
                    if not pi.valid:
                        self.census.add("invalidated_parent_merges_again" if parent_merged else "invalid_parent_merges")
                    if len(pi.lms) == len(pj.lms):
                        self.census.add("merge_equal_sizes")
                    if len(pi.lms) > len(pj.lms):                 # :864
                        self.census.add("merge_into_parent")
                        this, other = pi, pj
                    else:
                        self.census.add("merge_into_candidate")
                        this, other = pj, pi
                    self.merge(this, other)
                    planes_will_be_removed.append(other)
                    self.merges.append((this.row, other.row))
                    self.update_plane_via_RANSAC(this)
                    this.need = True
                    was_merged = True
                    parent_merged = True
                elif ao > offset_thr:
                    self.census.add("pair_far_offset_only")
                elif ad < self.dot_thr:
                    self.census.add("pair_far_angle_only")
                else:
                    self.census.add("pair_on_a_threshold")
                j += 1
        if was_merged:                                            # :889-895
            for pl in planes_will_be_removed:
                pl.in_db = False
                self.removed[pl.row] = self.removed.get(pl.row, 0) | 1
        return was_merged

    # -- refine_planes (:900-952)
    def refine_planes(self):
        was_changed = False
        planes_will_be_erased = []
        for plane in self.all_planes():
            if not plane.valid:
                self.census.add("refine_planes_invalid")
                planes_will_be_erased.append(plane)
                continue
            if plane.need:
                if self.update_plane_via_RANSAC(plane):
                    self.census.add("refine_planes_updated")
                    plane.need = False
                    was_changed = True
                else:
                    self.census.add("refine_planes_update_failed")
            elif len(plane.lms) < 2 * self.ppr:
                self.census.add("refine_planes_small")
                planes_will_be_erased.append(plane)
            else:
                self.census.add("refine_planes_kept")
        for pl in planes_will_be_erased:
            self.remove_landmarks_ownership(pl, "erase")
            pl.in_db = False
            self.removed[pl.row] = self.removed.get(pl.row, 0) | 2
        return was_changed

    # -- refine_points (:954-1004)
    def refine_points(self):
        was_changed = False
        seen = set()
        for plane in self.all_planes():
            if not plane.valid or plane.need or len(plane.lms) < self.ppr:
                continue
            lms = [lm for lm in plane.lms if not self.will_be_erased(lm) and self.owner[lm] >= 0]          # :970
            if seen & set(lms):
                self.census.add("point_moved_by_two_planes")
            seen |= set(lms)
            if not lms:
                continue
            pos, changed = PR.refine_points(self.pos[lms], np.zeros(len(lms), np.int32), np.full(len(lms), PR.LM_OWNED, np.uint8), [plane.eq], [1],
                                            self.dist_thresh)
            self.pos[lms] = pos
            self.lm_changed[lms] |= changed
            was_changed = was_changed or bool(changed.any())
        return was_changed


def run(t, g, dist_thresh, error_thresh, points_per_ransac=18, iters=50, dot_product_threshold=0.8, offset_delta_factor=6, seed=0, stages=STAGE_ALL):
    """Problem g of the tables t (arrays with a leading problem axis, not modified).  Returns (the Map as the call leaves it, outputs dict)."""
    m = Map(t, g, dist_thresh, error_thresh, points_per_ransac, iters, dot_product_threshold, offset_delta_factor, seed)
    o = dict(status=OK, was_merged=0, planes_changed=0, points_changed=0)
    m.census.add(f"stages_{stages}")
    try:
        if stages == STAGE_ALL and len(m.all_planes()) < 2:       # :777
            o["status"] = TOO_FEW_PLANES
            m.census.add("too_few_planes")
        else:
            if stages & STAGE_MERGE:
                o["was_merged"] = int(m.merge_planes())
            if stages & STAGE_PLANES:
                o["planes_changed"] = int(m.refine_planes())
            if stages & STAGE_POINTS:
                o["points_changed"] = int(m.refine_points())
    except Overflow:
        o["status"] = OVERFLOW
    o.update(num_merges=len(m.merges), merges=list(m.merges), num_updates=m.calls,
             removed=np.array([m.removed.get(r, 0) for r in range(len(m.planes))], np.uint8),
             update_status=np.array([m.update_status.get(r, NO_UPDATE) for r in range(len(m.planes))], np.uint8), lm_changed=m.lm_changed)
    return m, o


def expected(t, results, merge_cap):
    """(tables, outputs) of a call over these problems' results: tables from t, outputs from sentinel-filled arrays.  A problem that stopped with
    OVERFLOW has no defined tables: they are left as in t, and `defined` says which problems count."""
    G, NP = t["pl_state"].shape
    L = t["lm_owner"].shape[1]
    tab = {k: np.array(v, TABLE_DTYPES[k]) for k, v in t.items()}
    shape = dict(removed=(G, NP), merges=(G, merge_cap, 2), update_status=(G, NP), lm_changed=(G, L))
    out = {k: np.full(shape.get(k, (G,)), SENTINEL[k], DTYPES[k]) for k in SENTINEL}
    defined = np.ones(G, bool)
    for g, (m, o) in enumerate(results):
        for k in ("status", "was_merged", "planes_changed", "points_changed", "num_merges", "num_updates", "removed", "update_status", "lm_changed"):
            out[k][g] = o[k]
        for k, pair in enumerate(o["merges"][:merge_cap]):
            out["merges"][g, k] = pair
        if o["status"] == OVERFLOW:
            defined[g] = False
            continue
        for p in m.planes:
            tab["pl_state"][g, p.row] = p.state()
            tab["pl_equation"][g, p.row] = p.eq
            tab["pl_best_error"][g, p.row] = p.best_error
            tab["pl_lm"][g, p.row] = p.slots
        # a count outside [0, n_cap] is rewritten only where the list was
        for p in m.planes:
            if len(p.lms) != min(max(int(t["pl_count"][g, p.row]), 0), m.n_cap) or list(p.lms) != [int(x) for x in t["pl_lm"][g, p.row][:len(p.lms)]]:
                tab["pl_count"][g, p.row] = len(p.lms)
        tab["pos_w"][g] = m.pos
        tab["lm_owner"][g] = m.owner
    return tab, out, defined
