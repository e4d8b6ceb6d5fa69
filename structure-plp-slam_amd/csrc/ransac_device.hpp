// What the RANSAC kernels share on the device (sim3_kernels.hip, pnp_kernels.hip, essential_kernels.hip): the workgroup maximum of the
// best-hypothesis key and one step of an ordered compaction.  Workgroups of four waves (256 lanes) throughout.  The 16-lane Jacobi of
// pnp_kernels.hip and essential_kernels.hip is not here: as one template over the column count it compiled to other code than the two
// functions do (profiles/r30_ransac_core.md).
#pragma once
#include <hip/hip_runtime.h>

#include "plp_barrier.hpp"

namespace plp {

// the maximum of v over the workgroup; ends with the barrier behind which s_part may be rewritten
__device__ __forceinline__ unsigned long long wg_max_u64(unsigned long long v, unsigned long long (&s_part)[4]) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned long long o = __shfl_xor(v, d);
        v = o > v ? o : v;
    }
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = v;
    wg_barrier();
    unsigned long long m = s_part[0];
#pragma unroll
    for (int w = 1; w < 4; ++w) m = s_part[w] > m ? s_part[w] : m;
    wg_barrier();
    return m;
}

// One step of an ordered compaction over the workgroup: the position of this lane's item among the flagged ones (n before the step), and
// the new total.  Uniform over the workgroup; ends with a barrier.
// Not for sim3_kernels.hip's compact_slots or k_plane_hypotheses' two lists: they store into LDS before the closing barrier, which publishes the list.
__device__ __forceinline__ int wg_compact_step(bool v, int& n, int (&s_wave_n)[4]) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const unsigned long long m = __ballot(v);
    if (lane == 0) s_wave_n[w] = (int)__popcll(m);
    wg_barrier();
    int off = n, tot = 0;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        if (u < w) off += s_wave_n[u];
        tot += s_wave_n[u];
    }
    n += tot;
    wg_barrier();   // s_wave_n is rewritten by the next step
    return off + (int)__popcll(m & ((1ull << lane) - 1ull));
}

}  // namespace plp
