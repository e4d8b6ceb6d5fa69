// Map culling: module::local_map_cleaner (plp_cull_keyframes_* / plp_cull_landmarks_*, include/plp_front.h).  The steps
// are map_cull.hpp's, which the host build runs with a team of one lane; here, every workgroup 256 lanes:
//
// k_cull_count: a workgroup per entry of the flattened covisibility list.  A lane per key point of that key frame walks its landmark's
//      observation list once under the empty removed set; the two totals are integer LDS atomics and go to the context's count buffer
//      (-1, -1 for an entry the replay skips).  This is where the gathers are.
// k_cull_replay: a workgroup per problem walks its entries in order: the skip tests, the counts of k_cull_count while nothing is removed, a
//      recount against the removed set (a bitmap of F bits in LDS) after the first removal, the float decision, the bit behind a barrier.
// k_cull_dead_landmarks: the optional masks, grid (rows / 256, problems); the problem's final bitmap from the context's buffer into LDS, then
//      a lane per row: the bitmap's bit as a byte of out_kf_removed, and the same pass over a landmark's list for out_lm_erased.
// k_cull_landmark_states: a workgroup per fresh list, a lane per entry; the HOLD entries are ranked by ballot and wave prefix.
// The LDS state is reached through the shared structs alone, so no access is FLAT.
#include <hip/hip_runtime.h>

#include "plp_barrier.hpp"
#include "map_cull.hpp"

namespace plp {
namespace {

struct CullTeamWg {
    static constexpr int NT = kCullThreads, NW = kCullThreads / 64;
    __device__ __forceinline__ int tid() const { return threadIdx.x; }
    __device__ __forceinline__ int lane() const { return threadIdx.x & 63; }
    __device__ __forceinline__ int wave() const { return threadIdx.x >> 6; }
    __device__ __forceinline__ void barrier() const { wg_barrier(); }
    __device__ __forceinline__ unsigned long long ballot(bool v) const { return __ballot(v); }
    __device__ __forceinline__ void add(int32_t& t, int v) const { atomicAdd(&t, v); }
};

__global__ __launch_bounds__(kCullThreads) void k_cull_count(CullArgs A) {
    __shared__ CullShared sh;
    CullTeamWg par;
    cull_count_entry(A, blockIdx.x, sh, par);
}

__global__ __launch_bounds__(kCullThreads) void k_cull_replay(CullArgs A) {
    __shared__ CullShared sh;
    CullTeamWg par;
    cull_replay(A, blockIdx.x, sh, par);
}

__global__ __launch_bounds__(kCullThreads) void k_cull_dead_landmarks(CullArgs A) {
    __shared__ uint32_t rem[kCullWords];
    const int g = blockIdx.y;
    for (int i = threadIdx.x; i < A.words; i += kCullThreads) rem[i] = A.rem[(size_t)g * A.words + i];
    wg_barrier();
    cull_masks(A, g, blockIdx.x * kCullThreads + threadIdx.x, rem);
}

__global__ __launch_bounds__(kCullThreads) void k_cull_landmark_states(CullLmArgs A) {
    __shared__ CullSharedLm sh;
    CullTeamWg par;
    cull_states(A, blockIdx.x, sh, par);
}

}  // namespace

hipError_t launch_cull_keyframes(hipStream_t st, const CullArgs& A) {
    if (A.cnt && A.Cv > 0) hipLaunchKernelGGL(k_cull_count, dim3(A.Cv), dim3(kCullThreads), 0, st, A);
    hipLaunchKernelGGL(k_cull_replay, dim3(A.G), dim3(kCullThreads), 0, st, A);
    const int rows = cull_mask_rows(A);
    if (rows > 0) hipLaunchKernelGGL(k_cull_dead_landmarks, dim3((rows + kCullThreads - 1) / kCullThreads, A.G), dim3(kCullThreads), 0, st, A);
    return hipGetLastError();
}

hipError_t launch_cull_landmarks(hipStream_t st, const CullLmArgs& A) {
    hipLaunchKernelGGL(k_cull_landmark_states, dim3(A.R), dim3(kCullThreads), 0, st, A);
    return hipGetLastError();
}

}  // namespace plp
