// The matcher context (plp_matcher of include/plp_front.h) and what the files that implement its entry points share: match_context.hip and one
// *_context.hip per solver (sim3, pnp, essential, two_view, pose_opt, transform_opt, local_ba, local_map, plane, map_cull, covisibility, pose_graph, global_ba).
#pragma once
#include <hip/hip_runtime.h>

#include <mutex>

#include "plp_common.hpp"

struct plp_matcher {
    int device = 0;
    hipStream_t stream = nullptr;
    plp::DevBuf klist, klist2, kcount, claim, full_list, sorted, sorted_xr, row_start, dbg;  // scratch of the device path
    plp::DevBuf stage;                            // one slab for the host-pointer path
    plp::DevBuf bow_scratch;                      // plp_bow_query_device: the per-row arrays the caller did not ask for
    plp::DevBuf sim3_ctx, sim3_hyp;               // plp_sim3_ransac_device: what its launches hand to one another
    plp::DevBuf pnp_ctx, pnp_slot, pnp_hyp, pnp_corr, pnp_pose, pnp_sign;   // plp_pnp_ransac_device: likewise
    plp::DevBuf ess_ctx, ess_slot, ess_hyp, ess_pairs, ess_E, ess_code, ess_key;     // plp_essential_ransac_device: likewise
    plp::DevBuf tv_pts, tv_flag;                  // plp_two_view_pose_device: the points and flags of the four hypotheses
    plp::DevBuf pose_slot, pose_slot_lines, pose_chi2, pose_n;              // plp_pose_optimize_device: likewise
    plp::DevBuf tf_slot, tf_chi2, tf_n, tf_level, tf_edge;                                   // plp_transform_optimize_device: likewise
    plp::DevBuf la_d, la_i, la_b;                                                            // plp_local_ba_device: likewise
    plp::DevBuf lm_ws;                                                                       // plp_local_map_device: the mark table of a chunk of frames
    plp::DevBuf plane_hyp;                                                                   // plp_plane_ransac_device: the hypotheses' records
    plp::DevBuf cull_cnt, cull_rem;                                                          // plp_cull_keyframes_device: the snapshot counts, the removed sets
    plp::DevBuf pg_d, pg_i;                                                                  // plp_pose_graph_optimize_device: what its launches hand to one another
    plp::DevBuf covis_ws;                                                                    // plp_covisibility_update_device: what its two launches hand to one another
    plp::DevBuf gb_d, gb_i, gb_b, gb_S, gb_rec;                                              // plp_global_ba_device: the tables, the reduced system and the Levenberg record of the run
    plp::HostPinned gb_pin;                                                                  // ... and where the entry reads the record back
    plp::HostPinned pin;                          // page-locked staging of host images (post-extract depth)
    std::mutex mu;
};

// the camera of an entry is well-formed (match_context.hip; C linkage: the library has always exported this name)
extern "C" plp_status check_camera_model(const plp_camera_model* cam, bool depth_or_lines);

namespace {

// a kernel-argument table of 16 pyramid levels from the caller's num_levels floats (NULL: none), 1 past them
void fill_levels(float (&dst)[16], const float* src, int num_levels) {
    for (int i = 0; i < 16; ++i) dst[i] = (src && i < num_levels) ? src[i] : 1.0f;
}

// the camera fields reproject<MODEL> (reproject.hpp) reads, which ObserveArgs, ProjectArgs and KeypointPairArgs name alike
template <class Args> void set_camera(Args& A, const plp_camera_model& cm) {
    A.model = cm.model;
    A.fx = cm.fx; A.fy = cm.fy; A.cx = cm.cx; A.cy = cm.cy; A.fxb = cm.focal_x_baseline;
    A.cols_d = (double)(unsigned)cm.cols; A.rows_d = (double)(unsigned)cm.rows;
}

// The device entries' side of a solver's *_rooms() function, which names every context buffer of the solver once, with its element count, for
// both entries (the host-pointer entries pass a Stage, whose room() ignores the buffer): the buffer is reserved at count * sizeof(T), the
// pointer set, the first error kept and nothing reserved after it.
struct DeviceRooms {
    hipError_t err = hipSuccess;
    template <class T> void room(plp::DevBuf& buf, T*& p, size_t count) {
        if (err != hipSuccess) return;
        err = buf.reserve(count * sizeof(T));
        p = static_cast<T*>(buf.p);
    }
};

}  // namespace
