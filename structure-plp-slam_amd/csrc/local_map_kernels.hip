// The local map of B frames: module::local_map_updater (plp_local_map_*, include/plp_front.h).  The steps are
// local_map.hpp's, which the host build runs with a team of one lane; here:
//
// k_local_map_keyframes: a workgroup of 512 per frame.  The weights are integer LDS atomics into a table of F counters (F <= 8192: 32 KB), one lane
//      per slot of the frame walking that landmark's observation run; the first local key frames are compacted in ascending row by ballot and wave
//      prefix, `nearest` is the workgroup's maximum of weight << 32 | ~row; the second-order walk runs on wave 0 alone (ten lanes test the ten
//      covisibilities, the children go in tiles of 64, the first success is taken from the ballot) against a bitmap of the local rows in LDS.
// k_local_map_mark<LINES>: grid (local key frames + 1, frames of the chunk).  Every slot of local key frame k does an integer atomicMin of its
//      position k * cap + idx into the frame's row of the context's mark table (cleared to 0xFFFFFFFF on the stream); the last block sets a bit per
//      landmark the frame itself holds in the bitmap beside the table.
// k_local_map_compact<LINES>: a workgroup of 512 per frame walks the candidates in order; one is kept iff the table holds its own position (the
//      first-seen rule, for any kf_lm), and is ranked by ballot and prefix.
// The LDS tables are reached through the shared struct alone and the mark table through the kernel argument alone, so no access is FLAT.
#include <hip/hip_runtime.h>

#include "plp_barrier.hpp"
#include "local_map.hpp"

namespace plp {
namespace {

template <int THREADS> struct LmTeamWg {
    static constexpr int NT = THREADS, WS = 64, NW = THREADS / 64;
    __device__ __forceinline__ int tid() const { return threadIdx.x; }
    __device__ __forceinline__ int lane() const { return threadIdx.x & 63; }
    __device__ __forceinline__ int wave() const { return threadIdx.x >> 6; }
    __device__ __forceinline__ void barrier() const { wg_barrier(); }
    __device__ __forceinline__ unsigned long long ballot(bool v) const { return __ballot(v); }
    __device__ __forceinline__ void add(int32_t& t, int v) const { atomicAdd(&t, v); }
    __device__ __forceinline__ void bit_or(uint32_t& t, uint32_t v) const { atomicOr(&t, v); }
    __device__ __forceinline__ void min(uint32_t& t, uint32_t v) const { atomicMin(&t, v); }
};

__global__ __launch_bounds__(kLmThreads) void k_local_map_keyframes(LmArgs A) {
    __shared__ LmShared sh;
    LmTeamWg<kLmThreads> par;
    lm_keyframes(A, blockIdx.x, sh, par);
}

template <bool LINES> __global__ __launch_bounds__(kLmMarkThreads) void k_local_map_mark(LmArgs A) {
    LmTeamWg<kLmMarkThreads> par;
    lm_mark<LINES>(A, blockIdx.y, blockIdx.x, par);
}

template <bool LINES> __global__ __launch_bounds__(kLmThreads) void k_local_map_compact(LmArgs A) {
    __shared__ LmSharedCompact sh;
    LmTeamWg<kLmThreads> par;
    lm_compact<LINES>(A, blockIdx.x, sh, par);
}

}  // namespace

hipError_t launch_local_map_keyframes(hipStream_t st, const LmArgs& A) {
    hipLaunchKernelGGL(k_local_map_keyframes, dim3(A.B), dim3(kLmThreads), 0, st, A);
    return hipGetLastError();
}

hipError_t launch_local_map_lists(hipStream_t st, const LmArgs& A, bool lines) {
    const size_t tab = (size_t)A.nb * A.ws_rows * 4, bits = (size_t)A.nb * A.ws_words * 4;
    if (tab == 0) {                                   // no landmark row at all: the lists are empty, the counts still written
        if (lines) hipLaunchKernelGGL(k_local_map_compact<true>, dim3(A.nb), dim3(kLmThreads), 0, st, A);
        else hipLaunchKernelGGL(k_local_map_compact<false>, dim3(A.nb), dim3(kLmThreads), 0, st, A);
        return hipGetLastError();
    }
    hipError_t e = hipMemsetAsync(A.ws, 0xFF, tab, st);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(A.ws + (size_t)A.nb * A.ws_rows, 0, bits, st);
    if (e != hipSuccess) return e;
    const dim3 grid(lm_mark_blocks(A.k_cap, A.F) + 1, A.nb);
    if (lines) {
        hipLaunchKernelGGL(k_local_map_mark<true>, grid, dim3(kLmMarkThreads), 0, st, A);
        hipLaunchKernelGGL(k_local_map_compact<true>, dim3(A.nb), dim3(kLmThreads), 0, st, A);
    } else {
        hipLaunchKernelGGL(k_local_map_mark<false>, grid, dim3(kLmMarkThreads), 0, st, A);
        hipLaunchKernelGGL(k_local_map_compact<false>, dim3(A.nb), dim3(kLmThreads), 0, st, A);
    }
    return hipGetLastError();
}

}  // namespace plp
