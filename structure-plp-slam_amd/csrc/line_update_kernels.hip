// The line map update (plp_trim_line_endpoints_*, plp_correct_landmark_lines_*, plp_loop_ba_propagate_lines_*, include/plp_front.h; DESIGN.md
// section 5, D25).  The arithmetic and the statuses are line_update.hpp's, which the host build runs too; the file is compiled with
// -ffp-contract=off.
//
// One lane per line, 256 lanes a workgroup, no LDS, no barrier, no atomic.  A lane streams its own 48 B of Pluecker coordinates in and 48 B of
// coordinates or end points out, and gathers the rows of its reference key frame (the pose row, the two Sim3 rows, the key line) by ref_kf:
// lines of one key frame are neighbours in a map's tables more often than not, and a table of a thousand key frames (120 KB of pose rows) stays in
// L2, so the gathers cost latency, not HBM traffic.  k_trim_line_endpoints scans the line's observation list serially for its reference key frame
// (lists are short).  What bounds the kernels is the chain of f64 divisions of the trim and the 216 + 36 f64 products of the matrix product, per lane,
// not the bytes: profiles/r29_line_map_update.md.
#include <hip/hip_runtime.h>

#include "line_update.hpp"

namespace plp {
namespace {

__global__ __launch_bounds__(256) void k_trim_line_endpoints(LineTrimArgs A) {
    const int l = blockIdx.x * 256 + threadIdx.x;
    if (l < A.L) line_trim_item(A, l);
}

__global__ __launch_bounds__(256) void k_correct_landmark_lines(LineCorrectArgs A) {
    const int l = blockIdx.x * 256 + threadIdx.x;
    if (l < A.L) line_correct_item(A, l);
}

__global__ __launch_bounds__(256) void k_loop_ba_propagate_lines(LinePropagateArgs A) {
    const int l = blockIdx.x * 256 + threadIdx.x;
    if (l < A.L) line_propagate_item(A, l);
}

}  // namespace

hipError_t launch_trim_line_endpoints(hipStream_t st, const LineTrimArgs& A) {
    hipLaunchKernelGGL(k_trim_line_endpoints, dim3((A.L + 255) / 256), dim3(256), 0, st, A);
    return hipGetLastError();
}

hipError_t launch_correct_landmark_lines(hipStream_t st, const LineCorrectArgs& A) {
    hipLaunchKernelGGL(k_correct_landmark_lines, dim3((A.L + 255) / 256), dim3(256), 0, st, A);
    return hipGetLastError();
}

hipError_t launch_loop_ba_propagate_lines(hipStream_t st, const LinePropagateArgs& A) {
    hipLaunchKernelGGL(k_loop_ba_propagate_lines, dim3((A.L + 255) / 256), dim3(256), 0, st, A);
    return hipGetLastError();
}

}  // namespace plp
