// Place recognition (plp_bow_query_* / plp_bow_score_pairs_*, include/plp_front.h): data::bow_database::acquire_loop_candidates and
// acquire_relocalization_candidates (src/PLPSLAM/data/bow_database.cc:97-378) for Q queries against N database rows, and single scores for
// loop_detector::compute_min_score_in_covisibilities (module/loop_detector.cc:238-266).  Numeric contract: DESIGN.md section 5, D12; the
// score's terms and the two f32 thresholds are those of bow_score.hpp, which the host model runs too.
//
// The reference walks an inverted index word -> key frames to count the words a key frame shares with the query.  The count itself is
// |words(query) AND words(row)|, and here it is taken row by row:
//
// k_bow_count<true>   a workgroup owns one query and a run of rows.  It sets the query's words as bits in LDS (n_words bits, up to 160 KiB),
//                     then each wave streams a row's words coalesced, tests their bits and counts by ballot and popcount.
// k_bow_count<false>  the same for a vocabulary whose bitmap does not fit: the query's sorted words are staged in LDS (at most 32 KB) and
//                     every word of a row is searched by bisection.
// k_bow_select        max_common of a query over its candidates (one workgroup per query; the threshold follows from it in the readers).
// k_bow_score         one lane per row finds the rows above the threshold -- a handful per query -- and the wave scores them one after the
//                     other: 64 words of the row at a time, each lane bisects the query for its word and forms its term, and the terms of
//                     the common words are added to ONE accumulator in lane order, which is word order.  The chain is what makes the f64
//                     sum the reference's; it is as long as the row has common words.
// k_bow_totals        one workgroup per query: kept rows, totals over the covisibility lists, best_total, and the final mask.  The mask
//                     goes through a bitmap in LDS, a chunk of rows at a time, so that every byte of out_final has one writer and the waves
//                     exchange nothing through HBM.
// k_bow_score_pairs   one wave per pair, the scoring routine of k_bow_score.
// Nothing waits for the host between them: the threshold of a query is read from HBM by the next kernel on the stream.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bow_database.hpp"
#include "bow_score.hpp"
#include "plp_barrier.hpp"

namespace plp {
namespace {

constexpr int kBowFinalChunk = 8192 * 32;   // rows of the final mask one pass of k_bow_totals holds as bits in LDS

__device__ __forceinline__ int bow_clamp(int n, int cap) { return min(max(n, 0), cap); }

// the first index of the ascending list s[0 .. n) whose entry is not below w
template <class P> __device__ __forceinline__ int bow_lower_bound(P s, int n, uint32_t w) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (s[mid] < w) lo = mid + 1; else hi = mid;
    }
    return lo;
}

template <bool BITMAP>
__global__ __launch_bounds__(256) void k_bow_count(BowQueryArgs A, int rows_per_wg) {
    extern __shared__ uint32_t s_q[];   // BITMAP: (n_words + 31) / 32 dwords of bits; else the query's words, q_stride dwords
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), q = blockIdx.y;
    const int qn = bow_clamp(A.q_n[q], A.q_stride);
    const uint32_t* qw = A.q_word + (size_t)q * A.q_stride;
    if (BITMAP) {
        const int nd = (int)((A.n_words + 31u) >> 5);
        for (int i = tid; i < nd; i += 256) s_q[i] = 0u;
        wg_barrier();
        for (int i = tid; i < qn; i += 256) {
            const uint32_t w = qw[i];
            if (w < A.n_words) atomicOr(&s_q[w >> 5], 1u << (w & 31));
        }
    } else {
        for (int i = tid; i < qn; i += 256) s_q[i] = qw[i];
    }
    wg_barrier();
    const int r0 = blockIdx.x * rows_per_wg, r1 = min(A.N, r0 + rows_per_wg);
    for (int r = r0 + wave; r < r1; r += 4) {   // uniform over the wave
        const bool alive = !A.db_alive || A.db_alive[r] != 0;
        const int n = alive ? bow_clamp(A.db_n[r], A.stride) : 0;
        const uint32_t* row = A.db_word + (size_t)r * A.stride;
        int cnt = 0;
#pragma unroll 4
        for (int base = 0; base < n; base += 64) {
            const int i = base + lane;
            bool hit = false;
            if (i < n) {
                const uint32_t w = row[i];
                if (BITMAP) hit = w < A.n_words && ((s_q[w >> 5] >> (w & 31)) & 1u);
                else { const int p = bow_lower_bound(s_q, qn, w); hit = p < qn && s_q[p] == w; }
            }
            cnt += (int)__popcll(__ballot(hit));
        }
        if (lane == 0) A.common[(size_t)q * A.N + r] = (uint32_t)cnt;
    }
}

// candidate && thr < common: the rows compute_scores scores (bow_database.cc:294-296)
__device__ __forceinline__ bool bow_selected(const BowQueryArgs& A, size_t idx, uint32_t thr) {
    const uint32_t c = A.common[idx];
    return c > 0u && !(A.reject && A.reject[idx] != 0) && thr < c;
}

__global__ __launch_bounds__(256) void k_bow_select(BowQueryArgs A) {
    __shared__ uint32_t s_max[4];
    const int tid = threadIdx.x, q = blockIdx.x;
    uint32_t m = 0u;
    for (int k = tid; k < A.N; k += 256) {
        const size_t idx = (size_t)q * A.N + k;
        const uint32_t c = A.common[idx];
        if (c > 0u && !(A.reject && A.reject[idx] != 0)) m = max(m, c);   // init_candidates_ only (:120-126)
    }
    for (int o = 32; o > 0; o >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, o));
    if ((tid & 63) == 0) s_max[tid >> 6] = m;
    wg_barrier();
    if (tid == 0) A.max_common[q] = max(max(s_max[0], s_max[1]), max(s_max[2], s_max[3]));
}

__device__ __forceinline__ double bow_readlane_f64(double v, int src) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), src), hi = __builtin_amdgcn_readlane(__double2hiint(v), src);
    return __hiloint2double(hi, lo);
}

// L1Scoring::score(a, b) by one wave; every lane returns it.  b's words are taken 64 at a time; the terms of the common ones are added in
// lane order = ascending word order = the order of bow_l1_score
__device__ __forceinline__ double bow_wave_score(const uint32_t* wa, const double* va, int na, const uint32_t* wb, const double* vb, int nb, int lane) {
    double acc = 0.0;
    for (int base = 0; base < nb; base += 64) {   // uniform
        const int i = base + lane;
        bool hit = false;
        double term = 0.0;
        if (i < nb) {
            const uint32_t w = wb[i];
            const int p = bow_lower_bound(wa, na, w);
            if (p < na && wa[p] == w) { hit = true; term = bow_l1_term(va[p], vb[i]); }
        }
        unsigned long long m = __ballot(hit);
        while (m) {
            const int b = __builtin_amdgcn_readfirstlane((int)__ffsll((long long)m) - 1);
            m &= m - 1;
            acc += bow_readlane_f64(term, b);
        }
    }
    return bow_l1_finish(acc);
}

__global__ __launch_bounds__(256) void k_bow_score(BowQueryArgs A) {
    const int tid = threadIdx.x, lane = tid & 63, q = blockIdx.y, k = blockIdx.x * 256 + tid;
    const uint32_t thr = bow_min_common_words(A.max_common[q]);
    bool sel = false;
    if (k < A.N) {
        const size_t idx = (size_t)q * A.N + k;
        sel = bow_selected(A, idx, thr);
        if (!sel) A.score[idx] = -1.0f;
    }
    unsigned long long m = __ballot(sel);
    const int qn = bow_clamp(A.q_n[q], A.q_stride);
    const uint32_t* qw = A.q_word + (size_t)q * A.q_stride;
    const double* qv = A.q_value + (size_t)q * A.q_stride;
    while (m) {   // uniform over the wave
        const int b = __builtin_amdgcn_readfirstlane((int)__ffsll((long long)m) - 1);
        m &= m - 1;
        const int r = __builtin_amdgcn_readfirstlane(k - lane) + b;
        const int n = bow_clamp(A.db_n[r], A.stride);
        const double s = bow_wave_score(qw, qv, qn, A.db_word + (size_t)r * A.stride, A.db_value + (size_t)r * A.stride, n, lane);
        if (lane == 0) A.score[(size_t)q * A.N + r] = (float)s;   // const float score = bow_vocab_->score(...) (:301)
    }
}

__global__ __launch_bounds__(256) void k_bow_totals(BowQueryArgs A) {
    __shared__ uint32_t s_bits[kBowFinalChunk / 32];
    __shared__ float s_best[4];
    __shared__ int s_scored[4], s_kept[4], s_set[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, q = blockIdx.x;
    const float ms = A.min_score ? A.min_score[q] : 0.0f;
    const uint32_t mc = A.max_common[q], thr = bow_min_common_words(mc);
    const size_t row0 = (size_t)q * A.N;
    float best = ms;   // float best_total_score = min_score (:337)
    int n_scored = 0, n_kept = 0;
    for (int k = tid; k < A.N; k += 256) {
        const bool sel = bow_selected(A, row0 + k, thr);
        float tot = -1.0f;
        int bk = -1;
        if (sel) {
            ++n_scored;
            const float sc = A.score[row0 + k];
            if (ms <= sc) {   // (:323)
                ++n_kept;
                tot = sc;
                float bs = sc;
                bk = k;
                const int nc = A.n_covis ? bow_clamp(A.n_covis[k], A.covis_cap) : 0;
                for (int j = 0; j < nc; ++j) {   // (:354-367)
                    const int c = A.covis[(size_t)k * A.covis_cap + j];
                    if ((unsigned)c < (unsigned)A.N && bow_selected(A, row0 + c, thr)) {
                        const float s2 = A.score[row0 + c];
                        tot += s2;
                        if (bs < s2) { bs = s2; bk = c; }
                    }
                }
                if (best < tot) best = tot;   // (:371)
            }
        }
        A.total[row0 + k] = tot;
        A.best_kf[row0 + k] = bk;
    }
    for (int o = 32; o > 0; o >>= 1) {
        best = fmaxf(best, __shfl_xor(best, o));
        n_scored += __shfl_xor(n_scored, o);
        n_kept += __shfl_xor(n_kept, o);
    }
    if (lane == 0) { s_best[wave] = best; s_scored[wave] = n_scored; s_kept[wave] = n_kept; }
    wg_barrier();
    n_scored = s_scored[0] + s_scored[1] + s_scored[2] + s_scored[3];
    n_kept = s_kept[0] + s_kept[1] + s_kept[2] + s_kept[3];
    const int status = mc == 0u ? 1 : n_scored == 0 ? 2 : n_kept == 0 ? 3 : 0;
    best = status == 0 ? fmaxf(fmaxf(s_best[0], s_best[1]), fmaxf(s_best[2], s_best[3])) : ms;
    const float min_total = bow_min_total_score(best);
    int n_set = 0;
    for (int c0 = 0; c0 < A.N; c0 += kBowFinalChunk) {   // uniform over the workgroup
        const int cn = min(kBowFinalChunk, A.N - c0), nd = (cn + 31) >> 5;
        for (int i = tid; i < nd; i += 256) s_bits[i] = 0u;
        wg_barrier();
        if (status == 0) {
            for (int k = tid; k < A.N; k += 256) {   // the thread's own rows: it reads what it wrote above
                const int bk = A.best_kf[row0 + k];
                if (bk >= c0 && bk < c0 + cn && min_total < A.total[row0 + k]) atomicOr(&s_bits[(bk - c0) >> 5], 1u << ((bk - c0) & 31));   // (:156-165)
            }
        }
        wg_barrier();
        for (int i = tid; i < cn; i += 256) {
            const uint32_t bit = (s_bits[i >> 5] >> (i & 31)) & 1u;
            A.final_mask[row0 + c0 + i] = (uint8_t)bit;
            n_set += (int)bit;
        }
        wg_barrier();
    }
    for (int o = 32; o > 0; o >>= 1) n_set += __shfl_xor(n_set, o);
    if (lane == 0) s_set[wave] = n_set;
    wg_barrier();
    if (tid == 0) {
        if (A.n_final) A.n_final[q] = s_set[0] + s_set[1] + s_set[2] + s_set[3];
        if (A.best_total) A.best_total[q] = best;
        if (A.status) A.status[q] = (uint8_t)status;
    }
}

__global__ __launch_bounds__(256) void k_bow_score_pairs(BowPairsArgs A) {
    const int lane = threadIdx.x & 63, p = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);   // uniform over the wave
    if (p >= A.P) return;
    const int a = A.a_row[p], b = A.b_row[p];
    float out = -1.0f;
    if ((unsigned)a < (unsigned)A.NA && (unsigned)b < (unsigned)A.NB) {
        const int na = bow_clamp(A.a_n[a], A.stride_a), nb = bow_clamp(A.b_n[b], A.stride_b);
        out = (float)bow_wave_score(A.a_word + (size_t)a * A.stride_a, A.a_value + (size_t)a * A.stride_a, na, A.b_word + (size_t)b * A.stride_b,
                                    A.b_value + (size_t)b * A.stride_b, nb, lane);
    }
    if (lane == 0) A.out_score[p] = out;
}

}  // namespace

hipError_t launch_bow_query(hipStream_t st, const BowQueryArgs& A) {
    if (A.Q <= 0) return hipSuccess;
    if (A.N > 0) {
        // enough workgroups per query to fill the chip at Q = 1, at least one row per wave; the bitmap is cleared and set once per workgroup
        const int per_query = max(1, 1024 / A.Q), rows_per_wg = max(4, (A.N + per_query - 1) / per_query);
        const dim3 grid((A.N + rows_per_wg - 1) / rows_per_wg, A.Q);
        if (A.n_words <= kBowBitmapWords) {
            const size_t lds = (size_t)((A.n_words + 31u) >> 5) * 4;
            if (lds > 48 * 1024) {
                const hipError_t e = hipFuncSetAttribute((const void*)k_bow_count<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(kBowBitmapWords / 8));
                if (e != hipSuccess) return e;
            }
            hipLaunchKernelGGL(k_bow_count<true>, grid, dim3(256), lds, st, A, rows_per_wg);
        } else {
            hipLaunchKernelGGL(k_bow_count<false>, grid, dim3(256), (size_t)A.q_stride * 4, st, A, rows_per_wg);
        }
    }
    hipLaunchKernelGGL(k_bow_select, dim3(A.Q), dim3(256), 0, st, A);
    if (A.N > 0) hipLaunchKernelGGL(k_bow_score, dim3((A.N + 255) / 256, A.Q), dim3(256), 0, st, A);
    hipLaunchKernelGGL(k_bow_totals, dim3(A.Q), dim3(256), 0, st, A);
    return hipGetLastError();
}

hipError_t launch_bow_score_pairs(hipStream_t st, const BowPairsArgs& A) {
    if (A.P <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_bow_score_pairs, dim3((A.P + 3) / 4), dim3(256), 0, st, A);
    return hipGetLastError();
}

}  // namespace plp
