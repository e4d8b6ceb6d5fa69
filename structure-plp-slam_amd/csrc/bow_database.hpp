// Kernel arguments and launchers of the place-recognition entries (plp_bow_query_* / plp_bow_score_pairs_*, include/plp_front.h;
// bow_database_kernels.hip).  The arithmetic shared with the host is in bow_score.hpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace plp {

constexpr uint32_t kBowBitmapWords = 1310720;   // word ids a 160 KiB LDS bitmap holds: up to this n_words the count tests bits, above it bisects

struct BowQueryArgs {
    uint32_t n_words;
    int N, stride, Q, q_stride, covis_cap;
    const uint32_t* db_word; const double* db_value; const int32_t* db_n; const uint8_t* db_alive;
    const uint32_t* q_word; const double* q_value; const int32_t* q_n;
    const uint8_t* reject; const float* min_score;
    const int32_t* covis; const int32_t* n_covis;
    // [Q][N]: the caller's outputs or the context's scratch, never NULL when N > 0
    uint32_t* common; float* score; float* total; int32_t* best_kf; uint8_t* final_mask;
    // [Q]: max_common is never NULL; the others may be
    uint32_t* max_common; int32_t* n_final; float* best_total; uint8_t* status;
};

struct BowPairsArgs {
    int NA, stride_a, NB, stride_b, P;
    const uint32_t* a_word; const double* a_value; const int32_t* a_n;
    const uint32_t* b_word; const double* b_value; const int32_t* b_n;
    const int32_t* a_row; const int32_t* b_row;
    float* out_score;
};

hipError_t launch_bow_query(hipStream_t st, const BowQueryArgs& A);
hipError_t launch_bow_score_pairs(hipStream_t st, const BowPairsArgs& A);

}  // namespace plp
