// Host driver + C ABI of the matcher context: plane refinement: Planar_Mapping_module::refinement() over tables updated in place
// (include/plp_front.h: plp_plane_refinement_*; plane_refinement_kernels.hip, plane_refinement.hpp)
#include <hip/hip_runtime.h>

#include <vector>

#include "matcher_context.hpp"
#include "plane_refinement.hpp"

using namespace plp;

extern "C" {

namespace {
plp_status refinement_check(const plp_plane_refinement_args* a) {
    if (!a) return set_error(PLP_ERR_INVALID_ARG, "NULL argument");
    if (a->G < 0 || a->NP_cap < 0 || a->n_cap < 0 || a->L < 0 || a->merge_cap < 0) return set_error(PLP_ERR_INVALID_ARG, "G, NP_cap, n_cap, L and merge_cap must not be negative");
    if (a->points_per_ransac < 1 || a->iters < 1) return set_error(PLP_ERR_INVALID_ARG, "points_per_ransac and iters must be positive");
    if (a->stages < 1 || a->stages > 7) return set_error(PLP_ERR_INVALID_ARG, "stages must be a non-empty mask of PLP_PLANE_STAGE_*");
    if (a->n_cap > kPlaneMaxSlots) return set_error(PLP_ERR_UNSUPPORTED, "more than 8192 slots per plane");
    if (a->iters > kPlaneMaxIters) return set_error(PLP_ERR_UNSUPPORTED, "more than 1024 iterations");
    if (a->NP_cap > kPlaneRefMaxRows) return set_error(PLP_ERR_UNSUPPORTED, "more than 4096 plane rows per problem");
    if (a->G > 65535) return set_error(PLP_ERR_UNSUPPORTED, "more than 65535 problems in one call");
    if (a->G == 0) return PLP_OK;
    if (!a->dist_thresh || !a->error_thresh) return set_error(PLP_ERR_INVALID_ARG, "dist_thresh and error_thresh are required");
    if (!a->out_status || !a->out_was_merged || !a->out_planes_changed || !a->out_points_changed || !a->out_num_merges || !a->out_num_updates)
        return set_error(PLP_ERR_INVALID_ARG, "out_status, out_was_merged, out_planes_changed, out_points_changed, out_num_merges, out_num_updates are required");
    if (a->NP_cap > 0 && (!a->pl_state || !a->pl_equation || !a->pl_best_error || !a->pl_count || !a->out_removed || !a->out_update_status))
        return set_error(PLP_ERR_INVALID_ARG, "pl_state, pl_equation, pl_best_error, pl_count, out_removed, out_update_status are required");
    if (a->NP_cap > 0 && a->n_cap > 0 && !a->pl_lm) return set_error(PLP_ERR_INVALID_ARG, "pl_lm is required");
    if (a->L > 0 && (!a->pos_w || !a->lm_erased || !a->lm_owner || !a->out_lm_changed))
        return set_error(PLP_ERR_INVALID_ARG, "pos_w, lm_erased, lm_owner, out_lm_changed are required");
    if (a->merge_cap > 0 && !a->out_merges) return set_error(PLP_ERR_INVALID_ARG, "out_merges is required when merge_cap > 0");
    return PLP_OK;
}

PlaneRefArgs refinement_args(const plp_plane_refinement_args* a) {
    PlaneRefArgs A{};
    A.G = a->G; A.NP_cap = a->NP_cap; A.n_cap = a->n_cap; A.L = a->L; A.merge_cap = a->merge_cap; A.stages = a->stages;
    A.points_per_ransac = a->points_per_ransac; A.iters = a->iters; A.offset_delta_factor = a->offset_delta_factor; A.dot_thr = a->dot_product_threshold;
    A.seed = a->seed;
    A.pl_state = a->pl_state; A.pl_equation = a->pl_equation; A.pl_best_error = a->pl_best_error; A.pl_count = a->pl_count; A.pl_lm = a->pl_lm;
    A.pos_w = a->pos_w; A.lm_erased = a->lm_erased; A.lm_owner = a->lm_owner; A.dist_thresh = a->dist_thresh; A.error_thresh = a->error_thresh;
    A.out_status = a->out_status; A.out_was_merged = a->out_was_merged; A.out_planes_changed = a->out_planes_changed;
    A.out_points_changed = a->out_points_changed; A.out_removed = a->out_removed; A.out_num_merges = a->out_num_merges; A.out_merges = a->out_merges;
    A.out_num_updates = a->out_num_updates; A.out_update_status = a->out_update_status; A.out_lm_changed = a->out_lm_changed;
    return A;
}

// the arrays of the call; the rooms are what the waves of a workgroup hand to one another
extern "C++" template <class R> void refinement_plan(R& r, plp_matcher* c, PlaneRefArgs& A) {
    const size_t G = (size_t)A.G, NP = G * (size_t)A.NP_cap, L = G * (size_t)A.L;
    r.out(A.pl_state, NP); r.out(A.pl_equation, NP * 4); r.out(A.pl_best_error, NP); r.out(A.pl_count, NP); r.out(A.pl_lm, NP * (size_t)A.n_cap);
    r.out(A.pos_w, L * 3); r.in(A.lm_erased, L); r.out(A.lm_owner, L); r.in(A.dist_thresh, G); r.in(A.error_thresh, G);
    r.out(A.out_status, G, false); r.out(A.out_was_merged, G, false); r.out(A.out_planes_changed, G, false); r.out(A.out_points_changed, G, false);
    r.out(A.out_removed, NP, false); r.out(A.out_num_merges, G, false); r.out(A.out_merges, G * (size_t)A.merge_cap * 2);
    r.out(A.out_num_updates, G, false); r.out(A.out_update_status, NP, false); r.out(A.out_lm_changed, L, false);
    r.room(c->plane_ref_hyp, A.ctx_hyp, G * (size_t)A.iters * kPlaneHypDoubles);
    r.room(c->plane_ref_mark, A.ctx_mark, L + 1);
}
}  // namespace

plp_status plp_plane_refinement_device(plp_matcher* c, const plp_plane_refinement_args* a, void* hip_stream) {
    if (!c) return set_error(PLP_ERR_INVALID_ARG, "ctx is NULL");
    if (plp_status s = refinement_check(a)) return s;
    if (a->G == 0) return PLP_OK;
    return device_call(c, hip_stream, refinement_args(a), refinement_plan<DeviceRooms>, launch_plane_refinement);
}

plp_status plp_plane_refinement_host(plp_matcher* c, const plp_plane_refinement_args* a) {
    if (!c) return set_error(PLP_ERR_INVALID_ARG, "ctx is NULL");
    if (plp_status s = refinement_check(a)) return s;
    if (a->G == 0) return PLP_OK;
    return host_call(c, refinement_args(a), refinement_plan<Stage>, launch_plane_refinement);
}

// the host build of plane_refinement.hpp (no HIP call)
int32_t plp_model_plane_refinement_host(const plp_plane_refinement_args* a) {
    if (refinement_check(a) != PLP_OK) return -1;
    const PlaneRefArgs A = refinement_args(a);
    std::vector<uint8_t> mark((size_t)A.L, 0);
    for (int g = 0; g < A.G; ++g) plane_ref_model_problem(A, g, mark);
    return A.G;
}

}  // extern "C"
