// The covisibility graph: data::graph_node (plp_covisibility_update_* / plp_covisibility_erase_*, include/plp_front.h).
// The steps are covisibility.hpp's, which the host build runs with a team of one lane; here, every workgroup 256 lanes:
//
// k_covis_count: a workgroup per owner.  A lane per slot of the owner walks its landmark's observation list; the weights are integer LDS atomics
//      on a table of F counters.  The non-zero rows are compacted in ascending row by ballot and prefix, `nearest` is the workgroup's largest
//      weight << 13 | row, the pairs are ranked in LDS by the number of larger keys.  Base C and base O go to the context's scratch, not to the
//      tables: another owner's workgroup may still have to read this row as it was.  This is where the gathers are.
// k_covis_apply: a workgroup per key frame.  The base (its own from scratch, or the row as it stands) as a table of F weights in LDS; a lane per
//      owner looks the key frame up in that owner's base C (a bisection) and overlays the pair; then C by ballot and prefix, O by rank when an
//      overlay changed something, the parent and the status.  Writes its own row only and reads no row another workgroup writes.
// k_covis_erase: a workgroup per key frame, launched twice: the surviving rows (which read the erased ones), then the erased rows.
// The LDS state is reached through the shared struct alone, so no access is FLAT.
#include <hip/hip_runtime.h>

#include "plp_barrier.hpp"
#include "covisibility.hpp"

namespace plp {
namespace {

struct CvTeamWg {
    static constexpr int NT = kCvThreads, WS = 64, NW = kCvThreads / 64;
    __device__ __forceinline__ int tid() const { return threadIdx.x; }
    __device__ __forceinline__ int lane() const { return threadIdx.x & 63; }
    __device__ __forceinline__ int wave() const { return threadIdx.x >> 6; }
    __device__ __forceinline__ void barrier() const { wg_barrier(); }
    __device__ __forceinline__ unsigned long long ballot(bool v) const { return __ballot(v); }
    __device__ __forceinline__ void add(int32_t& t, int v) const { atomicAdd(&t, v); }
};

__global__ __launch_bounds__(kCvThreads) void k_covis_count(CvArgs A) {
    __shared__ CvShared sh;
    CvTeamWg par;
    cv_count(A, blockIdx.x, sh, par);
}

__global__ __launch_bounds__(kCvThreads) void k_covis_apply(CvArgs A) {
    __shared__ CvShared sh;
    CvTeamWg par;
    cv_apply(A, blockIdx.x, sh, par);
}

__global__ __launch_bounds__(kCvThreads) void k_covis_erase(CvArgs A) {
    __shared__ CvShared sh;
    CvTeamWg par;
    cv_erase(A, blockIdx.x, sh, par);
}

}  // namespace

hipError_t launch_covisibility_update(hipStream_t st, const CvArgs& A) {
    if (A.F > 0) {
        hipError_t e = hipMemsetAsync(A.pos_of, 0xFF, (size_t)A.F * sizeof(int32_t), st);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_covis_count, dim3(A.G), dim3(kCvThreads), 0, st, A);
    if (A.F > 0) hipLaunchKernelGGL(k_covis_apply, dim3(A.F), dim3(kCvThreads), 0, st, A);
    return hipGetLastError();
}

hipError_t launch_covisibility_erase(hipStream_t st, CvArgs A) {
    for (A.phase = 0; A.phase < 2; ++A.phase) hipLaunchKernelGGL(k_covis_erase, dim3(A.F), dim3(kCvThreads), 0, st, A);
    return hipGetLastError();
}

}  // namespace plp
