// What the RANSAC solvers share, one definition for host and device (sim3.hpp, pnp.hpp, essential.hpp, plane_fit.hpp; DESIGN.md section 5,
// D13): the sample generator, the choice between the caller's samples and drawn ones, the clamp of a problem's count and the packing of the
// best-hypothesis key.  Integer arithmetic only; needs nothing but <stdint.h> and the HIP attributes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace plp {

// splitmix64's finaliser
__host__ __device__ __forceinline__ uint64_t mix64(uint64_t x) {
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27; x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x;
}

// D13's counter-based generator: the stream of hypothesis `iter` of problem p under `seed`, r(k) = its k-th 32-bit number, k = 0, 1, ...
struct RansacStream {
    uint64_t base;
    __host__ __device__ __forceinline__ RansacStream(uint64_t seed, int p, int iter)
        : base(mix64(seed ^ mix64(((uint64_t)(uint32_t)p << 32) | (uint64_t)(uint32_t)iter))) {}
    __host__ __device__ __forceinline__ uint32_t r(int k) const { return (uint32_t)(mix64(base + (uint64_t)((uint32_t)k + 1u) * 0x9E3779B97F4A7C15ull) >> 32); }
};

// The samples the library draws when the caller passes none (D13): K distinct indices of [0, n), n >= K, by a partial Fisher-Yates shuffle
// of 0 .. n-1 (step k swaps position k with position k + r(k) mod (n - k)), the array kept as the few entries that moved.  Step k depends on
// the stream and k alone: the first K' of a K-draw are the K'-draw.
template <int K>
__host__ __device__ __forceinline__ void ransac_draw(uint64_t seed, int p, int iter, int n, int out[K]) {
    const RansacStream g(seed, p, iter);
    int idx[2 * K], val[2 * K];                                     // the moved entries, latest last
    int m = 0;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int j = k + (int)(g.r(k) % (uint32_t)(n - k));
        int aj = j, ak = k;                                         // a[j], a[k] as they stand
#pragma unroll
        for (int i = 0; i < 2 * K; ++i)
            if (i < m) {
                if (idx[i] == j) aj = val[i];
                if (idx[i] == k) ak = val[i];
            }
        out[k] = aj;
        idx[2 * k] = j; val[2 * k] = ak;                            // a[j] <- a[k]; a[k] <- a[j]
        idx[2 * k + 1] = k; val[2 * k + 1] = aj;
        m = 2 * k + 2;
    }
}

// the body of the plp_model_*_draw_host entries: the draws of iterations iter0 .. iter0 + n_iters - 1 of problem p, out n_iters x K.  Returns
// n_iters, or -1 for a bad argument.
template <int K>
inline int32_t ransac_draw_rows(uint64_t seed, int32_t p, int32_t iter0, int32_t n_iters, int32_t n, int32_t* out) {
    if (n_iters < 0 || n < K || (n_iters > 0 && !out)) return -1;
    for (int32_t i = 0; i < n_iters; ++i) {
        int idx[K];
        ransac_draw<K>(seed, p, iter0 + i, n, idx);
        for (int k = 0; k < K; ++k) out[K * (size_t)i + k] = idx[k];
    }
    return n_iters;
}

// sample k of the same stream as a rank of [0, n), n >= 1, with replacement (D19 item 2)
__host__ __device__ __forceinline__ int ransac_draw_one(uint64_t seed, int p, int iter, int k, int n) {
    return (int)(RansacStream(seed, p, iter).r(k) % (uint32_t)n);
}

// the K sample indices of hypothesis `iter` of problem p (the caller's, or drawn), and whether they name K distinct items of [0, n).  A: the
// solver's arguments, read by name: samples (P x iters x K, or NULL), iters, seed.
// The kernels' instruction streams are held to what the three solvers' own copies of this function compiled to (profiles/r30_ransac_core.md):
// hence plain pointers, not references to arrays, and the two cases written out -- they say what the loops say.
template <int K, class Args>
__host__ __device__ __forceinline__ bool ransac_sample(const Args& A, int p, int iter, int n, int idx[K]) {
    if (A.samples) {
        const int32_t* s = A.samples + ((size_t)p * A.iters + iter) * K;
        if constexpr (K == 4) {
            idx[0] = s[0]; idx[1] = s[1]; idx[2] = s[2]; idx[3] = s[3];
        } else {
#pragma unroll
            for (int a = 0; a < K; ++a) idx[a] = s[a];
        }
    } else {
        ransac_draw<K>(A.seed, p, iter, n, idx);
    }
    if constexpr (K == 3) {
        return (unsigned)idx[0] < (unsigned)n && (unsigned)idx[1] < (unsigned)n && (unsigned)idx[2] < (unsigned)n && idx[0] != idx[1] && idx[0] != idx[2] &&
               idx[1] != idx[2];
    }
    bool ok = true;
#pragma unroll
    for (int a = 0; a < K; ++a) {
        ok = ok && (unsigned)idx[a] < (unsigned)n;
#pragma unroll
        for (int b = a + 1; b < K; ++b) ok = ok && idx[a] != idx[b];
    }
    return ok;
}

// the number of slots of problem p that are in use: counts[p] cut to [0, cap], cap without a counts array
__host__ __device__ __forceinline__ int clamp_count(const int32_t* counts, int p, int cap) {
    if (!counts) return cap;
    const int n = counts[p];
    return n < 0 ? 0 : (n > cap ? cap : n);
}

// The best hypothesis of a problem is the maximum of this key: more (inliers, or score bits of a non-negative float) wins, among equals the
// lowest iteration.  What stands for "no hypothesis" is the solver's own affair (a count of 0; a key of 0).
__host__ __device__ __forceinline__ unsigned long long ransac_key(unsigned count_or_score_bits, int iter) {
    return ((unsigned long long)count_or_score_bits << 32) | (unsigned long long)(~(unsigned)iter);
}
__host__ __device__ __forceinline__ int ransac_key_iter(unsigned long long key) { return (int)(~(unsigned)key); }

}  // namespace plp
