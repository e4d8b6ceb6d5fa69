// Planar_Mapping_module::refinement() (planar_mapping_module.cc:773-793): merge_planes (:795-898), refine_planes (:900-952) and refine_points
// (:954-1004) over plane and landmark tables that are updated in place, one definition for host and device (plp_plane_refinement_* /
// plp_model_plane_refinement_host, include/plp_front.h; the reformulation: DESIGN.md section 4).  The arithmetic of
// an update is plane_fit.hpp's (D19's PLP_PLANE_UPDATE), reached through a Team; what this file adds is the pair test, the walk of the
// candidate loop, the state bytes and -- for the host build -- the three functions as serial loops (plane_refinement_kernels.hip holds the
// workgroup's form of the same steps).  Translation units that include this file are compiled with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "plane_fit.hpp"

namespace plp {

constexpr int kPlaneRefMaxRows = 4096;                // NP_cap limit: the state bytes and the compacted vector of a problem are LDS tables
constexpr int kPlaneRefNoUpdate = 255;                // out_update_status of a row no update touched

// what every problem of a call shares
struct PlaneRefArgs {
    int G, NP_cap, n_cap, L, merge_cap, stages, points_per_ransac, iters, offset_delta_factor;
    double dot_thr;
    unsigned long long seed;
    uint8_t* pl_state; double* pl_equation; double* pl_best_error; int32_t* pl_count; int32_t* pl_lm;
    double* pos_w; const uint8_t* lm_erased; int32_t* lm_owner; const double* dist_thresh; const double* error_thresh;
    uint8_t* out_status; uint8_t* out_was_merged; uint8_t* out_planes_changed; uint8_t* out_points_changed; uint8_t* out_removed;
    int32_t* out_num_merges; int32_t* out_merges; int32_t* out_num_updates; uint8_t* out_update_status; uint8_t* out_lm_changed;
    double* ctx_hyp;                                  // DEVICE, G x iters x kPlaneHypDoubles: the hypotheses of the update that runs
    uint8_t* ctx_mark;                                // DEVICE, G x L: the parent's members during a merge, 0 between merges
};
hipError_t launch_plane_refinement(hipStream_t st, const PlaneRefArgs& A);   // plane_refinement_kernels.hip: one launch

// the outcome of the two-sided test of a pair (:850-860)
enum { kPlanePairFar = 0, kPlanePairMerge = 1, kPlanePairMixed = 2 };
__host__ __device__ __forceinline__ int plane_pair_test(const double pi[4], const double pj[4], double offset_thr, double dot_thr) {
    const double ni = 1.0 / plane_abs_n(pi), nj = 1.0 / plane_abs_n(pj);                     // :842-843
    const double offset_delta = pi[3] * ni - pj[3] * nj;                                     // :850
    const double dot = plane_dot(pi, pj) * (ni * nj);                                        // :851
    const double ao = __builtin_fabs(offset_delta), ad = __builtin_fabs(dot);
    if (ao > offset_thr && ad < dot_thr) return kPlanePairFar;                               // :853
    if (ao < offset_thr && ad > dot_thr) return kPlanePairMerge;                             // :859
    return kPlanePairMixed;
}

// Whether the candidate loop (:826-835) tests entry j, given that `before` entries directly in front of j, back to where the loop entered
// (i + 1, or the entry after a merge), are invalid: a valid j always (the for's own step, or the step over one invalid entry); an invalid
// j when the step over its predecessor lands on it, i.e. at an odd offset into its run of invalid entries.
__host__ __device__ __forceinline__ bool plane_candidate_tested(bool valid, int before) { return valid || (before & 1) != 0; }

// the flag byte D19 reads for a slot (:623-628, :656): an entry that names no landmark counts as erased
__host__ __device__ __forceinline__ uint8_t plane_slot_flag(const PlaneRefArgs& A, size_t lbase, int lm) {
    if ((unsigned)lm >= (unsigned)A.L) return (uint8_t)PLP_PLANE_LM_ERASED;
    return (uint8_t)((A.lm_erased[lbase + lm] ? PLP_PLANE_LM_ERASED : 0) | (A.lm_owner[lbase + lm] >= 0 ? PLP_PLANE_LM_OWNED : 0));
}

// set_invalid() (:604, :724) and set_need_refinement() (:700) of an update, on the row's state byte
__host__ __device__ __forceinline__ uint8_t plane_state_after_update(uint8_t st, int flags) {
    if (flags & PLP_PLANE_FLAG_INVALID) st = (uint8_t)(st & ~PLP_PLANE_ROW_VALID);
    if (flags & PLP_PLANE_FLAG_NEED_REFINEMENT) st = (uint8_t)(st | PLP_PLANE_ROW_NEED_REFINEMENT);
    return st;
}

// the fields of D19's argument block that plane_early_status and plane_refit_gate read
__host__ __device__ __forceinline__ PlaneArgs plane_update_args(const PlaneRefArgs& A) {
    PlaneArgs U{};
    U.mode = PLP_PLANE_UPDATE; U.points_per_ransac = A.points_per_ransac; U.iters = A.iters; U.n_cap = A.n_cap;
    return U;
}

// whether refine_points works on a row (:960-962)
__host__ __device__ __forceinline__ bool plane_row_active(uint8_t st, int count, int points_per_ransac) {
    return (st & PLP_PLANE_ROW_IN_DB) != 0 && (st & PLP_PLANE_ROW_VALID) != 0 && (st & PLP_PLANE_ROW_NEED_REFINEMENT) == 0 && count >= points_per_ransac;
}

// ---- the host build: one problem, one plane, one hypothesis and one point after the other

// update_plane_via_RANSAC (:593-733) of `row`, the c-th update call of problem g: D19's status
inline int plane_ref_model_update(const PlaneRefArgs& A, int g, int row, int c) {
    const size_t prow = (size_t)g * A.NP_cap + row, lbase = (size_t)g * A.L;
    const int n = clamp_count(A.pl_count, (int)prow, A.n_cap), I = A.iters;
    int32_t* lst = A.pl_lm + prow * A.n_cap;
    const double* pos = A.pos_w + 3 * lbase;
    const PlaneArgs U = plane_update_args(A);
    std::vector<int> lm((size_t)n), elig, live;
    std::vector<uint8_t> fl((size_t)n);
    for (int s = 0; s < n; ++s) {
        lm[s] = lst[s];
        fl[s] = plane_slot_flag(A, lbase, lm[s]);
        if (plane_eligible(PLP_PLANE_UPDATE, fl[s])) elig.push_back(s);
        if (plane_live(fl[s])) live.push_back(s);
    }
    const int n_elig = (int)elig.size();
    int flags = 0;
    const int early = plane_early_status(U, n, n_elig, flags);
    A.out_update_status[prow] = (uint8_t)early;
    if (early != PLP_PLANE_OK) {
        A.pl_state[prow] = plane_state_after_update(A.pl_state[prow], flags);
        return early;
    }
    const int m = plane_sample_size(PLP_PLANE_UPDATE, n, A.points_per_ransac);
    const double thr = A.dist_thresh[g], error_thresh = A.error_thresh[g];
    PlaneHostTeam T;
    std::vector<double> eq_s((size_t)4 * I), eq_r((size_t)4 * I, 0.0), res((size_t)I), err((size_t)I, kPlaneMax);
    std::vector<uint8_t> tried((size_t)I, 0);
    std::vector<int> list;
    for (int it = 0; it < I; ++it) {
        int sweeps;
        plane_fit(T, [&](int k, double x[3]) {
            const int rank = ransac_draw_one(A.seed + (unsigned long long)g, c, it, k, n_elig);
            if ((unsigned)rank >= (unsigned)n_elig) return false;
            const double* w = pos + 3 * (size_t)lm[elig[rank]];
            x[0] = w[0]; x[1] = w[1]; x[2] = w[2];
            return true;
        }, m, &eq_s[4 * (size_t)it], res[it], sweeps);
        const double abs_n = plane_abs_n(&eq_s[4 * (size_t)it]);
        list.clear();
        for (int s : live)
            if (plane_distance(&eq_s[4 * (size_t)it], abs_n, pos + 3 * (size_t)lm[s]) < thr) list.push_back(s);
        tried[it] = plane_refit_gate(U, n, (int)list.size()) ? 1 : 0;
        if (tried[it])
            plane_fit(T, [&](int k, double x[3]) {
                const double* w = pos + 3 * (size_t)lm[list[k]];
                x[0] = w[0]; x[1] = w[1]; x[2] = w[2];
                return true;
            }, (int)list.size(), &eq_r[4 * (size_t)it], err[it], sweeps);
    }
    const PlaneReplay R = plane_replay(PLP_PLANE_UPDATE, I, A.pl_best_error[prow], error_thresh, [&](int i) { return res[i]; },
                                       [&](int i) { return tried[i] != 0; }, [&](int i) { return err[i]; });
    int status = plane_late_status(PLP_PLANE_UPDATE, R, error_thresh, flags);
    const double* eq = R.last_refit ? &eq_r[4 * (size_t)R.last_iter] : &eq_s[4 * (size_t)R.last_iter];
    std::vector<int> members;
    if (status == PLP_PLANE_OK) {                                                          // step [4] (:704-720)
        const double* eq_b = &eq_s[4 * (size_t)R.best_iter];
        const double abs_b = plane_abs_n(eq_b), abs_n = plane_abs_n(eq);
        for (int s : live)
            if (plane_distance(eq_b, abs_b, pos + 3 * (size_t)lm[s]) < thr && plane_distance(eq, abs_n, pos + 3 * (size_t)lm[s]) < thr) members.push_back(lm[s]);
        if ((int)members.size() < A.points_per_ransac) { status = PLP_PLANE_TOO_FEW_LEFT; flags = PLP_PLANE_FLAG_INVALID; }   // :722
    }
    for (int i = 0; i < 4; ++i) A.pl_equation[4 * prow + i] = eq[i];
    A.pl_best_error[prow] = R.plane_error;
    A.pl_state[prow] = plane_state_after_update(A.pl_state[prow], flags);
    A.out_update_status[prow] = (uint8_t)status;
    if (status == PLP_PLANE_OK) {                                                          // :728-730
        for (int s = 0; s < n; ++s)
            if ((unsigned)lm[s] < (unsigned)A.L) A.lm_owner[lbase + lm[s]] = -1;
        for (size_t k = 0; k < members.size(); ++k) { lst[k] = members[k]; A.lm_owner[lbase + members[k]] = row; }
        A.pl_count[prow] = (int32_t)members.size();
    }
    return status;
}

// One problem.  mark: L bytes of 0, left as they were.
inline void plane_ref_model_problem(const PlaneRefArgs& A, int g, std::vector<uint8_t>& mark) {
    const size_t pbase = (size_t)g * A.NP_cap, lbase = (size_t)g * A.L;
    uint8_t* st = A.pl_state + pbase;
    int status = PLP_PLANE_REFINEMENT_OK, num_merges = 0, num_updates = 0;
    bool was_merged = false, planes_changed = false, points_changed = false;
    std::vector<int> all;                                                                  // get_all_landmark_planes()
    for (int r = 0; r < A.NP_cap; ++r) {
        if (st[r] & PLP_PLANE_ROW_IN_DB) all.push_back(r);
        A.out_removed[pbase + r] = 0;
        A.out_update_status[pbase + r] = (uint8_t)kPlaneRefNoUpdate;
    }
    for (int l = 0; l < A.L; ++l) A.out_lm_changed[lbase + l] = 0;
    const int n_db = (int)all.size();
    if (A.stages == 7 && n_db < 2) status = PLP_PLANE_REFINEMENT_TOO_FEW_PLANES;              // :777
    if (status == PLP_PLANE_REFINEMENT_OK && (A.stages & PLP_PLANE_STAGE_MERGE) && n_db >= 2) {   // :799-808
        const double offset_thr = (double)A.offset_delta_factor * A.dist_thresh[g];           // :813
        std::vector<int> removed;
        for (int i = 0; i < n_db && status == PLP_PLANE_REFINEMENT_OK; ++i) {
            const int ri = all[i];
            if (!(st[ri] & PLP_PLANE_ROW_VALID)) continue;                                     // :820
            int before = 0;                                                                    // invalid entries directly in front of j
            for (int j = i + 1; j < n_db; ++j) {
                const int rj = all[j];
                const bool valid = (st[rj] & PLP_PLANE_ROW_VALID) != 0;
                const bool tested = plane_candidate_tested(valid, before);                     // :828-835
                before = valid ? 0 : before + 1;
                if (!tested) continue;
                if (plane_pair_test(A.pl_equation + 4 * (pbase + ri), A.pl_equation + 4 * (pbase + rj), offset_thr, A.dot_thr) != kPlanePairMerge) continue;
                const int ci = clamp_count(A.pl_count, (int)(pbase + ri), A.n_cap), cj = clamp_count(A.pl_count, (int)(pbase + rj), A.n_cap);
                const int parent = ci > cj ? ri : rj, other = ci > cj ? rj : ri;               // :864
                // Plane::merge (landmark_plane.cc:221-248)
                int32_t* pl = A.pl_lm + (pbase + parent) * A.n_cap;
                const int32_t* ol = A.pl_lm + (pbase + other) * A.n_cap;
                int np = ci > cj ? ci : cj;
                const int no = ci > cj ? cj : ci;
                for (int s = 0; s < np; ++s)
                    if ((unsigned)pl[s] < (unsigned)A.L) mark[pl[s]] = 1;
                int fresh = 0;
                for (int s = 0; s < no; ++s)
                    if ((unsigned)ol[s] < (unsigned)A.L && !A.lm_erased[lbase + ol[s]] && !mark[ol[s]]) ++fresh;
                if (np + fresh > A.n_cap) {
                    status = PLP_PLANE_REFINEMENT_OVERFLOW;
                } else {
                    for (int s = 0; s < no; ++s)                                               // remove_landmarks_ownership() (:233)
                        if ((unsigned)ol[s] < (unsigned)A.L) A.lm_owner[lbase + ol[s]] = -1;
                    const int np0 = np;
                    for (int s = 0; s < no; ++s) {                                             // :235-242
                        const int lm = ol[s];
                        if ((unsigned)lm >= (unsigned)A.L || A.lm_erased[lbase + lm]) continue;
                        if (!mark[lm]) pl[np++] = lm;
                        A.lm_owner[lbase + lm] = parent;
                    }
                    A.pl_count[pbase + parent] = np;
                    st[parent] = (uint8_t)(st[parent] | PLP_PLANE_ROW_NEED_REFINEMENT);         // :244
                    st[other] = (uint8_t)(st[other] & ~PLP_PLANE_ROW_VALID);                   // :247
                    np = np0;
                }
                for (int s = 0; s < np; ++s)
                    if ((unsigned)pl[s] < (unsigned)A.L) mark[pl[s]] = 0;
                if (status != PLP_PLANE_REFINEMENT_OK) break;
                removed.push_back(other);                                                      // :867, :876
                if (num_merges < A.merge_cap) {
                    A.out_merges[2 * ((size_t)g * A.merge_cap + num_merges)] = parent;
                    A.out_merges[2 * ((size_t)g * A.merge_cap + num_merges) + 1] = other;
                }
                ++num_merges;
                plane_ref_model_update(A, g, parent, num_updates++);                           // :870, :879
                st[parent] = (uint8_t)(st[parent] | PLP_PLANE_ROW_NEED_REFINEMENT);             // :871, :880
                was_merged = true;
                before = 0;                                                                    // the walk goes on behind j as if entered there
            }
        }
        if (status == PLP_PLANE_REFINEMENT_OK)
            for (int r : removed) {                                                            // :889-895
                st[r] = (uint8_t)(st[r] & ~PLP_PLANE_ROW_IN_DB);
                A.out_removed[pbase + r] |= 1;
            }
    }
    if (status == PLP_PLANE_REFINEMENT_OK && (A.stages & PLP_PLANE_STAGE_REFINE_PLANES)) {
        std::vector<int> erase;
        for (int r = 0; r < A.NP_cap; ++r) {
            if (!(st[r] & PLP_PLANE_ROW_IN_DB)) continue;
            if (!(st[r] & PLP_PLANE_ROW_VALID)) { erase.push_back(r); continue; }              // :907-911
            if (st[r] & PLP_PLANE_ROW_NEED_REFINEMENT) {
                if (plane_ref_model_update(A, g, r, num_updates++) == PLP_PLANE_OK) {          // :917
                    st[r] = (uint8_t)(st[r] & ~PLP_PLANE_ROW_NEED_REFINEMENT);
                    planes_changed = true;
                }
            } else if (clamp_count(A.pl_count, (int)(pbase + r), A.n_cap) < 2 * A.points_per_ransac) {
                erase.push_back(r);                                                            // :926-929
            }
        }
        for (int r : erase) {                                                                  // :934-941
            const int n = clamp_count(A.pl_count, (int)(pbase + r), A.n_cap);
            const int32_t* lst = A.pl_lm + (pbase + r) * A.n_cap;
            for (int s = 0; s < n; ++s)
                if ((unsigned)lst[s] < (unsigned)A.L) A.lm_owner[lbase + lst[s]] = -1;
            st[r] = (uint8_t)(st[r] & ~PLP_PLANE_ROW_IN_DB);
            A.out_removed[pbase + r] |= 2;
        }
    }
    if (status == PLP_PLANE_REFINEMENT_OK && (A.stages & PLP_PLANE_STAGE_REFINE_POINTS)) {
        const double thr = A.dist_thresh[g];
        for (int r = 0; r < A.NP_cap; ++r) {
            const int n = clamp_count(A.pl_count, (int)(pbase + r), A.n_cap);
            if (!plane_row_active(st[r], n, A.points_per_ransac)) continue;                    // :960-965
            const double* eq = A.pl_equation + 4 * (pbase + r);
            const int32_t* lst = A.pl_lm + (pbase + r) * A.n_cap;
            for (int s = 0; s < n; ++s) {
                const int lm = lst[s];
                const uint8_t f = plane_slot_flag(A, lbase, lm);
                if (!plane_live(f) || !(f & PLP_PLANE_LM_OWNED)) continue;                     // :970
                double* x = A.pos_w + 3 * (lbase + lm);
                if (plane_refine_point(eq, thr, x)) { A.out_lm_changed[lbase + lm] = 1; points_changed = true; }
            }
        }
    }
    A.out_status[g] = (uint8_t)status;
    A.out_was_merged[g] = was_merged ? 1 : 0; A.out_planes_changed[g] = planes_changed ? 1 : 0; A.out_points_changed[g] = points_changed ? 1 : 0;
    A.out_num_merges[g] = num_merges; A.out_num_updates[g] = num_updates;
}

}  // namespace plp
