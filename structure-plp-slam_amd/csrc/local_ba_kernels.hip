// Local bundle adjustment: optimize::local_bundle_adjuster (plp_local_ba_*, include/plp_front.h).  The steps are
// local_ba.hpp's, which the host build runs with a team of one lane; here the team is a workgroup of 512 lanes (kLaThreads), one workgroup per
// problem, three launches:
//
// k_la_prepare: the roles of the key frames and landmarks from the tables (LDS flags), the edges of every local landmark's run of the
//      observation list with their measurements, the vertices' estimates, the free key frames ranked in table order (ballot + wave prefix).
// k_la_solve:   both rounds without the host.  Per round the active sets and every active pose's edge list (a wave per pose scans the edge
//      table with ballots).  A pass gives every edge one lane (f64 error and both Jacobian blocks, the terms into the edge table); a landmark's
//      sums belong to one lane that walks its run, a pose's 27 sums to 27 lanes that walk its list, a chain over the landmarks goes through an
//      LDS tile that lane 0 adds in order.  The Schur complement gives every coefficient of the reduced system to one lane (item (i, r, c) walks
//      pose i's edges and their landmarks' runs); the Cholesky works column by column with one barrier per column, row p being lane p's.
//      The system lives in the context's buffers (L2); only those are touched here.
// k_la_finish:  step [7]'s verdict for every edge and the outputs.
#include <hip/hip_runtime.h>

#include "local_ba_team.hpp"

namespace plp {
namespace {

__global__ __launch_bounds__(kLaThreads) void k_la_prepare(LaArgs A) {
    __shared__ LaShared sh;
    LaTeamWg par;
    la_prepare(A, blockIdx.x, sh, par);
}

__global__ __launch_bounds__(kLaThreads) void k_la_solve(LaArgs A) {
    __shared__ LaShared sh;
    LaTeamWg par;
    la_solve(A, blockIdx.x, sh, par);
}

__global__ __launch_bounds__(kLaThreads) void k_la_finish(LaArgs A) {
    LaTeamWg par;
    la_finish(A, blockIdx.x, par);
}

}  // namespace

hipError_t launch_local_ba(hipStream_t st, const LaArgs& A) {
    hipLaunchKernelGGL(k_la_prepare, dim3(A.G), dim3(kLaThreads), 0, st, A);
    hipLaunchKernelGGL(k_la_solve, dim3(A.G), dim3(kLaThreads), 0, st, A);
    hipLaunchKernelGGL(k_la_finish, dim3(A.G), dim3(kLaThreads), 0, st, A);
    return hipGetLastError();
}

}  // namespace plp
