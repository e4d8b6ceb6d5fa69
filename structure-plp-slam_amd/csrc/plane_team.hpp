// A wave as the Team of a fit of plane_fit.hpp (D19 item 4): lane j owns partial chain j, the 64 partials are chained in lane order by reading
// the lanes one after the other.  Shared by the kernels of plane_kernels.hip and plane_refinement_kernels.hip.
#pragma once
#include <hip/hip_runtime.h>

namespace plp {
namespace {

struct PlaneWaveTeam {
    int lane;
    double* work;                                     // kPlaneWorkDoubles of LDS
    template <int N, class F> __device__ __forceinline__ void sum64(F f, double (&tot)[N]) {
        double part[N];
#pragma unroll
        for (int i = 0; i < N; ++i) part[i] = 0.0;
        f(lane, part);
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const int lo = __double2loint(part[i]), hi = __double2hiint(part[i]);
            double t = 0.0;
#pragma unroll 8
            for (int j = 0; j < 64; ++j)                  // lane j's partial through scalar registers: j is uniform
                t = t + __hiloint2double(__builtin_amdgcn_readlane(hi, j), __builtin_amdgcn_readlane(lo, j));
            tot[i] = t;
        }
    }
    __device__ __forceinline__ bool leader() const { return lane == 0; }
    __device__ __forceinline__ double* jacobi_work() { return work; }
    __device__ __forceinline__ double share(double v) const { return __shfl(v, 0); }
    __device__ __forceinline__ int share(int v) const { return __shfl(v, 0); }
};

}  // namespace
}  // namespace plp
