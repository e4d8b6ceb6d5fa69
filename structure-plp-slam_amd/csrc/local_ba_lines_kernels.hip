// Local bundle adjustment with line landmarks: optimize::local_bundle_adjuster_extended_line (plp_local_ba_lines_*, include/plp_front.h;
// DESIGN.md section 5, D28).  The steps are local_ba_lines.hpp's, which the host build runs with a team of one lane; here the team is a
// workgroup of 512 lanes (kLaThreads), one workgroup per problem, four launches: local_ba_kernels.hip's three with one launch per round, so
// that each round's kernel holds its scalar registers.
//
// k_ll_prepare: k_la_prepare's work, then the local lines, the key frames fixed through a line and the line edges with their measurements.
// k_ll_solve<ROUND>: one round without the host; round 2 takes the kept buffer, the chi2 and lambda of round 1 from the problem's header.
//      Beside k_la_solve's tables a round keeps the twelve perturbed poses of every active free key frame and the eight perturbed copies of
//      every active line, formed once per linearisation; a line edge's lane evaluates its 21 errors in one loop over those tables.  A line's
//      sums belong to one lane that walks its run; a pose's 27 sums go on over its line edges; the chains go on over the lines through the
//      same LDS tile; every coefficient of the reduced system takes its line subtractions behind its landmark ones.
// k_ll_finish:  k_la_finish's work, then step [7]'s verdict for every line edge and the lines' outputs.
#include <hip/hip_runtime.h>

#include "local_ba_team.hpp"
#include "local_ba_lines.hpp"

namespace plp {
namespace {

__global__ __launch_bounds__(kLaThreads) void k_ll_prepare(LlArgs A) {
    __shared__ LlShared sh;
    LaTeamWg par;
    ll_prepare(A, blockIdx.x, sh, par);
}

template <int ROUND> __global__ __launch_bounds__(kLaThreads) void k_ll_solve(LlArgs A) {
    __shared__ LlShared sh;
    LaTeamWg par;
    ll_solve_round<ROUND>(A, blockIdx.x, sh, par);
}

__global__ __launch_bounds__(kLaThreads) void k_ll_finish(LlArgs A) {
    LaTeamWg par;
    ll_finish(A, blockIdx.x, par);
}

}  // namespace

hipError_t launch_local_ba_lines(hipStream_t st, const LlArgs& A) {
    hipLaunchKernelGGL(k_ll_prepare, dim3(A.p.G), dim3(kLaThreads), 0, st, A);
    hipLaunchKernelGGL(k_ll_solve<0>, dim3(A.p.G), dim3(kLaThreads), 0, st, A);
    hipLaunchKernelGGL(k_ll_solve<1>, dim3(A.p.G), dim3(kLaThreads), 0, st, A);
    hipLaunchKernelGGL(k_ll_finish, dim3(A.p.G), dim3(kLaThreads), 0, st, A);
    return hipGetLastError();
}

}  // namespace plp
