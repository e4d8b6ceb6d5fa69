// The arithmetic of data::bow_database (src/PLPSLAM/data/bow_database.cc:97-378) that has to be the same on the host and on the device: the
// similarity score of two BowVectors and the two f32 thresholds.  Compiled for both (bow_database_kernels.hip, plp_model_bow_score_host,
// tools/bow_score_sanitized.cpp).  Numeric contract: DESIGN.md section 5, D12.
//
// The score is DBoW2's L1Scoring::score (bow_vocab_->score with the ORB vocabulary's L1_NORM).  DBoW2 is not in the reference tree: this is
// restated from the published algorithm, as the transform is -- PARITY UNPINNED.  Both maps are walked in ascending word order; every word
// they share adds  fabs(v - w) - fabs(v) - fabs(w)  (v: the first vector's value, w: the second's; the two subtractions left to right) to ONE
// f64 accumulator in that order, and the score is -acc / 2.0.  There is no multiply in a term, so nothing can contract; the order of the
// additions is the only freedom, and it is fixed.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PLP_BOW_HD __host__ __device__ inline
#else
#define PLP_BOW_HD inline
#endif

namespace plp {

// one common word's term: v from the first argument of score(), w from the second
PLP_BOW_HD double bow_l1_term(double v, double w) { return fabs(v - w) - fabs(v) - fabs(w); }
PLP_BOW_HD double bow_l1_finish(double acc) { return -acc / 2.0; }

// L1Scoring::score(a, b) over two sorted (word, value) lists, sequentially: the definition the kernels' ordered sum is held to
PLP_BOW_HD double bow_l1_score(const uint32_t* wa, const double* va, int32_t na, const uint32_t* wb, const double* vb, int32_t nb) {
    double acc = 0.0;
    int32_t i = 0, j = 0;
    while (i < na && j < nb) {
        if (wa[i] == wb[j]) { acc += bow_l1_term(va[i], vb[j]); ++i; ++j; }
        else if (wa[i] < wb[j]) ++i;
        else ++j;
    }
    return bow_l1_finish(acc);
}

// min_num_common_words = static_cast<unsigned int>(0.8f * max_num_common_words): an f32 product (bow_database.cc:127, :196)
PLP_BOW_HD uint32_t bow_min_common_words(uint32_t max_common) { return (uint32_t)(0.8f * (float)max_common); }
// min_total_score = 0.75f * best_total_score (:153, :221)
PLP_BOW_HD float bow_min_total_score(float best_total) { return 0.75f * best_total; }

}  // namespace plp
