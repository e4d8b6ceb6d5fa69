// The team of the local adjusters' kernels (local_ba_kernels.hip, local_ba_lines_kernels.hip): a workgroup of 512 lanes (kLaThreads) in waves of
// 64, where the host build runs the same steps with LaTeamHost, a team of one lane.
#pragma once
#include <hip/hip_runtime.h>

#include "plp_barrier.hpp"
#include "local_ba.hpp"

namespace plp {

struct LaTeamWg {
    static constexpr int NT = kLaThreads, WS = 64, NW = kLaThreads / 64;
    __device__ __forceinline__ int tid() const { return threadIdx.x; }
    __device__ __forceinline__ int lane() const { return threadIdx.x & 63; }
    __device__ __forceinline__ int wave() const { return threadIdx.x >> 6; }
    __device__ __forceinline__ void barrier() const { wg_barrier(); }
    __device__ __forceinline__ void barrier_g() const { wg_barrier_after_global_stores(); }
    __device__ __forceinline__ unsigned long long ballot(bool v) const { return __ballot(v); }
    __device__ __forceinline__ void add(int32_t& t, int v) const { atomicAdd(&t, v); }
};

}  // namespace plp
