// Loop closing: optimize::graph_optimizer's pose graph (plp_pose_graph_optimize_*, plp_correct_landmarks_*, include/plp_front.h; DESIGN.md
// section 5, D22).  The steps are pose_graph.hpp's, which the host build runs with a team of one lane; here the team is a workgroup of 512
// lanes (kPgThreads), one workgroup per problem, three launches:
//
// k_pg_prepare: the vertices' estimates, the loop connections compacted in list order (ballot + wave prefix), the edges of [3.2] -- every
//      key frame counts its edges, a prefix over the rows, every key frame writes its own -- and the structure of the system: the vertices of
//      the system in row order, first(i), the skyline's offsets, every vertex's edge list in insertion order.
// k_pg_solve:   all iterations without the host.  A pass gives every edge one lane (the error and up to 28 perturbed errors, f64); a
//      coefficient of the skyline or of b belongs to one lane that walks its vertex's edge list; chi2, the largest diagonal and computeScale
//      are chains through an LDS tile that lane 0 adds in order; the Cholesky of the skyline works column by column with one barrier per
//      column, row p being lane p's, and so do both substitutions.  The skyline, the edge table and the estimates live in the context's
//      buffers (L2 / HBM); the offsets into them and the index tables of the vertices sit in LDS.
// k_pg_finish:  the outputs.
// k_pg_correct_landmarks: the landmark half, one lane per landmark.
#include <hip/hip_runtime.h>

#include "plp_barrier.hpp"
#include "pose_graph.hpp"

namespace plp {
namespace {

struct PgTeamWg {
    static constexpr int NT = kPgThreads, NW = kPgThreads / 64;
    __device__ __forceinline__ int tid() const { return threadIdx.x; }
    __device__ __forceinline__ int lane() const { return threadIdx.x & 63; }
    __device__ __forceinline__ int wave() const { return threadIdx.x >> 6; }
    __device__ __forceinline__ void barrier() const { wg_barrier(); }
    __device__ __forceinline__ void barrier_g() const { wg_barrier_after_global_stores(); }
    __device__ __forceinline__ unsigned long long ballot(bool v) const { return __ballot(v); }
};

__global__ __launch_bounds__(kPgThreads) void k_pg_prepare(PgArgs A) {
    __shared__ PgShared sh;
    PgTeamWg par;
    pg_prepare(A, blockIdx.x, sh, par);
}

__global__ __launch_bounds__(kPgThreads) void k_pg_solve(PgArgs A) {
    __shared__ PgShared sh;
    PgTeamWg par;
    pg_solve(A, blockIdx.x, sh, par);
}

__global__ __launch_bounds__(kPgThreads) void k_pg_finish(PgArgs A) {
    PgTeamWg par;
    pg_finish(A, blockIdx.x, par);
}

__global__ __launch_bounds__(256) void k_pg_correct_landmarks(PgLmArgs A) {
    const int l = blockIdx.x * 256 + threadIdx.x;
    if (l < A.L) pg_correct_landmark(A, l);
}

}  // namespace

hipError_t launch_pose_graph(hipStream_t st, const PgArgs& A) {
    hipLaunchKernelGGL(k_pg_prepare, dim3(A.G), dim3(kPgThreads), 0, st, A);
    hipLaunchKernelGGL(k_pg_solve, dim3(A.G), dim3(kPgThreads), 0, st, A);
    hipLaunchKernelGGL(k_pg_finish, dim3(A.G), dim3(kPgThreads), 0, st, A);
    return hipGetLastError();
}

hipError_t launch_correct_landmarks(hipStream_t st, const PgLmArgs& A) {
    hipLaunchKernelGGL(k_pg_correct_landmarks, dim3((A.L + 255) / 256), dim3(256), 0, st, A);
    return hipGetLastError();
}

}  // namespace plp
