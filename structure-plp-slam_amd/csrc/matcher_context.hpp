// The matcher context (plp_matcher of include/plp_front.h) and what the files that implement its entry points share: match_context.hip and one
// *_context.hip per solver (sim3, pnp, essential, two_view, perspective_init, pose_opt, transform_opt, local_ba, local_ba_lines, local_map, plane, plane_refinement, map_cull,
// covisibility, pose_graph, global_ba, line_update).
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
    plp::DevBuf persp_ctx, persp_norm, persp_T, persp_slot, persp_hyp, persp_pairs, persp_M, persp_code, persp_key;   // plp_perspective_ransac_device: likewise
    plp::DevBuf persp_pts, persp_flag;            // plp_perspective_pose_device: the points and flags of the eight hypotheses
    plp::DevBuf pose_slot, pose_slot_lines, pose_chi2, pose_n;              // plp_pose_optimize_device: likewise
    plp::DevBuf tf_slot, tf_chi2, tf_n, tf_level, tf_edge;                                   // plp_transform_optimize_device: likewise
    plp::DevBuf la_d, la_i, la_b;                                                            // plp_local_ba_device: likewise
    plp::DevBuf lm_ws;                                                                       // plp_local_map_device: the mark table of a chunk of frames
    plp::DevBuf plane_hyp;                                                                   // plp_plane_ransac_device: the hypotheses' records
    plp::DevBuf plane_ref_hyp, plane_ref_mark;                                               // plp_plane_refinement_device: the records of the update that runs, the marks of a merge
    plp::DevBuf cull_cnt, cull_rem;                                                         // plp_cull_keyframes_device: the snapshot counts, the removed sets
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

// Every entry of the context names the arrays of its call once, in a plan: a callable (R& r, plp_matcher* c, Args& A), usually a function template
// xx_plan<R>, that declares every pointer field of A in the order the call lists it: r.in (read), r.out (written; keep, Stage's comment in
// plp_common.hpp), r.room (a context buffer the launches hand work through).  The two forms of the entry run the same plan with two receivers:
// DeviceRooms for the device form, whose arrays are the caller's device memory, and plp::Stage for the host-pointer form, which stages every
// declared array through the context's slab.

// The device form's receiver: in and out do nothing; room reserves the context's buffer at count * sizeof(T) and sets the pointer, the first
// error is kept and nothing reserved after it.
struct DeviceRooms {
    hipError_t err = hipSuccess;
    template <class T> void in(const T*&, size_t) {}
    template <class T> void out(T*&, size_t, bool = true) {}
    template <class T> void room(plp::DevBuf& buf, T*& p, size_t count) {
        if (err != hipSuccess) return;
        err = buf.reserve(count * sizeof(T));
        p = static_cast<T*>(buf.p);
    }
};

// the last entry of an offset list (NULL: 0), a count only the host-pointer form can read and only that form needs: for the plan of a call
// whose array sizes stand in such a list.  Called before upload(), while the list is still the caller's host memory.
inline size_t list_end(const plp::Stage&, const int32_t* offsets, int n) { return offsets ? (size_t)offsets[n] : 0; }
inline size_t list_end(const DeviceRooms&, const int32_t*, int) { return 0; }

// a call without an argument struct or without an array to declare (the image entries, which have a device form only)
struct NoArgs {};
struct NoArrays { template <class R, class Args> void operator()(R&, plp_matcher*, Args&) const {} };

// what a run answers, as the entry's status: a launch_* function gives the first hipError_t of its launches, a run of several steps a plp_status
inline plp_status run_status(plp_status s) { return s; }
inline plp_status run_status(hipError_t launch_error) { PLP_HIP(launch_error); return PLP_OK; }

// The two scaffolds, one per form of an entry, called once the entry has checked its arguments and answered an empty call (neither takes the
// lock nor calls HIP).  They are the only places that know which lock is held, which device is set and which stream runs the call.  run is a
// callable (hipStream_t, Args&), mostly the launch_* function itself; work that needs the rooms' device addresses belongs in it.
// Device form: the caller's arrays are device memory and the call is queued on the caller's stream; the scaffold waits for nothing.
template <class Args, class Plan, class Run> plp_status device_call(plp_matcher* c, void* hip_stream, Args A, Plan plan, Run run) {
    std::lock_guard<std::mutex> lk(c->mu);
    PLP_HIP(hipSetDevice(c->device));
    DeviceRooms r;
    plan(r, c, A);
    PLP_HIP(r.err);
    return run_status(run((hipStream_t)hip_stream, A));
}

// Host-pointer form: the plan's arrays go through the context's slab and the call runs on the context's stream; finish() is the one wait.
template <class Args, class Plan, class Run> plp_status host_call(plp_matcher* c, Args A, Plan plan, Run run) {
    std::lock_guard<std::mutex> lk(c->mu);
    PLP_HIP(hipSetDevice(c->device));
    plp::Stage s(c->stage, c->stream);
    plan(s, c, A);
    PLP_TRY(s.upload());
    PLP_TRY(run_status(run(c->stream, A)));
    return s.finish();
}

}  // namespace
