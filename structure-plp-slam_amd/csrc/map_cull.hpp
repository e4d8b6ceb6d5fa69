// module::local_map_cleaner (module/local_map_cleaner.cc:51-320): remove_redundant_keyframes for G current key frames over one map snapshot and
// remove_redundant_landmarks[_line] for R fresh lists: one definition for host and device (plp_cull_keyframes_* / plp_cull_landmarks_* /
// plp_model_cull_*_host, include/plp_front.h).  Integers, and the two float comparisons of the text.
//
// The steps are written once over a team `P` of lanes, as local_map.hpp's are (its helpers and its team of one serve here too): the kernels run
// them with a workgroup, the host build with a team of one.  No result depends on the team's size: the counts are integer sums and every list
// position is a rank in list order.
//
//   cull_count      (num_valid, num_redundant) of count_redundant_observations (:242-320) for one key frame under a set of removed key frames:
//                   a lane per key point, one pass over its landmark's observation list
//   cull_replay     per problem: the loop of :212-237 in list order; the removed set is a bitmap of the team's shared state
//   cull_masks      per (problem, row): the removed set as bytes, and the landmarks dead under the problem's final removed set
//   cull_states     per fresh list: the state of every entry (:72-110) and the HOLD entries compacted in order
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/plp_front.h"
#include "local_map.hpp"

namespace plp {

constexpr int kCullMaxKf = kLmMaxKf;          // F: the removed set is a bitmap of kCullMaxKf bits of shared state
constexpr int kCullMaxSlots = kLmMaxSlots;    // cap
constexpr int kCullMaxProblems = 65535;       // G: the y extent of k_cull_dead_landmarks' grid
constexpr int kCullThreads = 256;             // every workgroup of map_cull_kernels.hip
constexpr int kCullWords = kCullMaxKf / 32;

struct CullArgs {
    int F, L, T, cap, kp_stride, G, Cv, mono;
    uint32_t origin_id;
    const int32_t* kf_lm; const int32_t* kf_counts; const plp_keypoint* undist; const float* x_right; const float* depths; const float* depth_thr;
    const uint32_t* kf_id; const uint8_t* kf_cannot_erase;
    const int32_t* obs_offsets; const int32_t* obs_kf; const int32_t* obs_idx; const uint8_t* lm_erased; const uint32_t* lm_num_obs;
    const int32_t* cur_kf; const int32_t* covis_offsets; const int32_t* covis;
    int32_t* out_num_removed; uint8_t* out_decision; int32_t* out_num_valid; int32_t* out_num_redundant; uint8_t* out_kf_removed; uint8_t* out_lm_erased;
    // what the context owns: the counts of every entry under the empty removed set ([Cv][2], -1 = not counted; NULL = the replay counts alone)
    // and every problem's final removed set ([G][words], NULL unless out_kf_removed or out_lm_erased is given)
    int32_t* cnt; uint32_t* rem; int words;
};

struct CullShared {
    uint32_t rem[kCullWords];                 // the removed set R of D20
    int32_t nv, nr;                           // the totals of one cull_count
};

__host__ __device__ __forceinline__ bool cull_bit(const uint32_t* rem, int kf) { return (rem[kf >> 5] >> (kf & 31)) & 1u; }

// one pass over the observation list of `lm` (D20): n0 by the 2 / 1 rule of landmark.cc:84-97 (or lm_num_obs), the weight of the observers in
// `rem` (landmark.cc:99-136; any_removed = 0: the set is empty and is not looked at), whether there is one, and the observers left other than
// row `self` whose octave is at most oct + 1 (:289-313).  An observation whose key frame or index is outside the tables counts as absent.
struct CullObs { uint32_t live; bool dead; int better; };
__host__ __device__ __forceinline__ CullObs cull_observations(const CullArgs& A, int lm, const uint32_t* rem, bool any_removed, int self, int oct) {
    int lo, hi;
    lm_run(A.obs_offsets, lm, A.T, lo, hi);
    uint32_t n0 = 0, gone = 0;
    bool any = false;
    int better = 0;
    for (int t = lo; t < hi; ++t) {
        const int kf = A.obs_kf[t], idx = A.obs_idx[t];
        if ((unsigned)kf >= (unsigned)A.F || (unsigned)idx >= (unsigned)A.cap) continue;
        const size_t at = (size_t)kf * A.kp_stride + idx;
        const uint32_t w = (A.x_right && 0 <= A.x_right[at]) ? 2u : 1u;
        n0 += w;
        if (any_removed && cull_bit(rem, kf)) { gone += w; any = true; continue; }
        if (kf != self && self >= 0 && A.undist[at].octave <= oct + 1) ++better;
    }
    if (A.lm_num_obs) n0 = A.lm_num_obs[lm];
    CullObs o;
    o.live = n0 - gone;
    o.dead = any && o.live <= 2u;                                     // the discard of landmark.cc:125-134, cumulative: counts only fall
    o.better = better;
    return o;
}

// ---- count_redundant_observations (:242-320) of key frame row c with the key frames of sh.rem removed (any_removed = 0: none); the totals in sh.nv, sh.nr
template <class P> __host__ __device__ __forceinline__ void cull_count(const CullArgs& A, int c, bool any_removed, CullShared& sh, P& par) {
    if (par.tid() == 0) { sh.nv = 0; sh.nr = 0; }
    par.barrier();
    const int cnt = lm_count(A.kf_counts, c, A.cap);
    int nv = 0, nr = 0;
    for (int idx = par.tid(); idx < cnt; idx += P::NT) {
        const int lm = A.kf_lm[(size_t)c * A.cap + idx];
        if (!lm_present(lm, A.L, A.lm_erased)) continue;                 // !lm, will_be_erased(), :255-262
        const size_t at = (size_t)c * A.kp_stride + idx;
        if (!A.mono) {                                                   // :265-269 (a NaN depth passes)
            const float depth = A.depths[at];
            if (depth < 0.0f || A.depth_thr[c] < depth) continue;
        }
        const CullObs o = cull_observations(A, lm, sh.rem, any_removed, c, A.undist[at].octave);
        if (o.dead) continue;                                            // erase_landmark_with_index made the slot a nullptr
        ++nv;
        if (o.live <= 3u) continue;                                      // :274
        if (o.better >= 3) ++nr;                                         // :305
    }
    if (nv) par.add(sh.nv, nv);
    if (nr) par.add(sh.nr, nr);
    par.barrier();
}

// the problem of flattened entry j: the last g with covis_offsets[g] <= j, or -1 when j is not inside that problem's run
__host__ __device__ __forceinline__ int cull_problem_of(const CullArgs& A, int j) {
    int lo = 0, hi = A.G;                                                // the answer is in [lo, hi)
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        if (A.covis_offsets[mid] <= j) lo = mid; else hi = mid;
    }
    return (A.covis_offsets[lo] <= j && j < A.covis_offsets[lo + 1]) ? lo : -1;
}

// the two skip tests (:214-223) and the row checks of entry c of a problem whose current key frame is in the table (cur_ok) with id id_cur: a
// PLP_CULL_KF_* skip code, or -1
__host__ __device__ __forceinline__ int cull_skip(const CullArgs& A, bool cur_ok, uint32_t id_cur, int c) {
    if ((unsigned)c >= (unsigned)A.F || !cur_ok) return PLP_CULL_KF_ABSENT;
    const uint32_t id_c = A.kf_id[c];
    if (id_c == A.origin_id) return PLP_CULL_KF_SKIP_ORIGIN;
    if (id_c <= id_cur && id_cur <= id_c + 2u) return PLP_CULL_KF_SKIP_WINDOW;
    return -1;
}

// ---- the counts of flattened entry j under the empty removed set, into A.cnt
template <class P> __host__ __device__ __forceinline__ void cull_count_entry(const CullArgs& A, int j, CullShared& sh, P& par) {
    const int g = cull_problem_of(A, j);
    bool skip = g < 0;
    if (!skip) {
        const int cur = A.cur_kf[g];
        const bool cur_ok = (unsigned)cur < (unsigned)A.F;
        skip = cull_skip(A, cur_ok, cur_ok ? A.kf_id[cur] : 0u, A.covis[j]) >= 0;
    }
    if (skip) {
        if (par.tid() == 0) { A.cnt[2 * (size_t)j] = -1; A.cnt[2 * (size_t)j + 1] = -1; }
        return;
    }
    cull_count(A, A.covis[j], false, sh, par);
    if (par.tid() == 0) { A.cnt[2 * (size_t)j] = sh.nv; A.cnt[2 * (size_t)j + 1] = sh.nr; }
}

// ---- remove_redundant_keyframes (:201-240) of problem g
template <class P> __host__ __device__ __forceinline__ void cull_replay(const CullArgs& A, int g, CullShared& sh, P& par) {
    const int tid = par.tid();
    for (int i = tid; i < A.words; i += P::NT) sh.rem[i] = 0;
    par.barrier();
    int lo, hi;
    lm_run(A.covis_offsets, g, A.Cv, lo, hi);
    const int cur = A.cur_kf[g];
    const bool cur_ok = (unsigned)cur < (unsigned)A.F;
    const uint32_t id_cur = cur_ok ? A.kf_id[cur] : 0u;
    int num_removed = 0;
    bool any = false;                                                    // R is not empty
    for (int j = lo; j < hi; ++j) {
        const int c = A.covis[j];
        const int skip = cull_skip(A, cur_ok, id_cur, c);
        if (skip >= 0) {
            if (tid == 0) A.out_decision[j] = (uint8_t)skip;
            continue;
        }
        int nv = -1, nr = -1;
        if (!any && A.cnt) { nv = A.cnt[2 * (size_t)j]; nr = A.cnt[2 * (size_t)j + 1]; }
        if (nv < 0) {
            // two copies of the count, each with the set's test resolved: one copy that carries `any` spills more scalar registers
            if (any) cull_count(A, c, true, sh, par); else cull_count(A, c, false, sh, par);
            nv = sh.nv; nr = sh.nr;
            par.barrier();                                               // every lane has the totals before the next count clears them
        }
        // :232, in float; 0 / 0 is NaN and keeps the key frame
        const bool removed = 0.9f <= (float)(uint32_t)nr / (float)(uint32_t)nv;
        const bool held = removed && A.kf_cannot_erase && A.kf_cannot_erase[c];   // prepare_for_erasing returns early (keyframe.cc:880-884)
        if (tid == 0) {
            A.out_decision[j] = (uint8_t)(!removed ? PLP_CULL_KF_KEPT : held ? PLP_CULL_KF_REMOVED_HELD : PLP_CULL_KF_REMOVED);
            A.out_num_valid[j] = nv; A.out_num_redundant[j] = nr;
            if (removed && !held) sh.rem[c >> 5] |= 1u << (c & 31);
        }
        if (removed) ++num_removed;
        if (removed && !held) { any = true; par.barrier(); }             // the bit is set before the next count reads the set
    }
    par.barrier();
    if (tid == 0) A.out_num_removed[g] = num_removed;
    if (A.rem)
        for (int i = tid; i < A.words; i += P::NT) A.rem[(size_t)g * A.words + i] = sh.rem[i];
}

// ---- the optional masks of problem g from its final removed set `rem`, for row i of either table: out_kf_removed is the set as bytes; a point
// landmark is dead at the end of the loop iff it was erased before it or the cascade discarded it
__host__ __device__ __forceinline__ void cull_masks(const CullArgs& A, int g, int i, const uint32_t* rem) {
    if (A.out_kf_removed && i < A.F) A.out_kf_removed[(size_t)g * A.F + i] = (uint8_t)cull_bit(rem, i);
    if (A.out_lm_erased && i < A.L) {
        bool dead = A.lm_erased && A.lm_erased[i];
        if (!dead) dead = cull_observations(A, i, rem, true, -1, 0).dead;
        A.out_lm_erased[(size_t)g * A.L + i] = (uint8_t)dead;
    }
}
// rows of cull_masks: the longer of the tables asked for
__host__ __device__ __forceinline__ int cull_mask_rows(const CullArgs& A) {
    const int f = A.out_kf_removed ? A.F : 0, l = A.out_lm_erased ? A.L : 0;
    return f > l ? f : l;
}

struct CullLmArgs {
    int R, N, L;
    const int32_t* fresh_offsets; const int32_t* fresh; const uint8_t* lm_erased; const uint32_t* num_observed; const uint32_t* num_observable;
    const uint32_t* first_kf_id; const uint32_t* num_obs; const uint8_t* owning_plane; const uint32_t* cur_kf_id; const uint32_t* num_obs_thr;
    uint8_t* out_state; int32_t* out_num_removed; int32_t* out_num_fresh; int32_t* out_fresh;
};

// lm_state of :72-110 (and :154-178, whose landmarks own no plane); a row outside the table leaves the buffer like an erased one
__host__ __device__ __forceinline__ int cull_state(const CullLmArgs& A, int lm, uint32_t cur, uint32_t thr) {
    if (!lm_present(lm, A.L, A.lm_erased)) return PLP_CULL_DROP;                              // :73
    const bool plane = A.owning_plane && A.owning_plane[lm];
    const float ratio = (float)A.num_observed[lm] / (float)A.num_observable[lm];              // landmark.cc:453-457
    if (ratio < 0.3f) return plane ? PLP_CULL_DROP : PLP_CULL_ERASE;                          // :79-91
    const uint32_t first = A.first_kf_id[lm];
    if (2u + first <= cur && A.num_obs[lm] <= thr) return plane ? PLP_CULL_DROP : PLP_CULL_ERASE;   // :92-104
    if (2u + 1u + first <= cur) return PLP_CULL_DROP;                                         // :105-110
    return PLP_CULL_HOLD;
}

struct CullSharedLm { int32_t wave_n[kCullThreads / 64]; int32_t removed; };

// ---- fresh list r: the states, the HOLD entries in order inside the list's own run of out_fresh, both counts
template <class P> __host__ __device__ __forceinline__ void cull_states(const CullLmArgs& A, int r, CullSharedLm& sh, P& par) {
    int lo, hi;
    lm_run(A.fresh_offsets, r, A.N, lo, hi);
    if (par.tid() == 0) sh.removed = 0;
    par.barrier();
    const uint32_t cur = A.cur_kf_id[r], thr = A.num_obs_thr[r];
    int n = 0, removed = 0;
    for (int base = lo; base < hi; base += P::NT) {
        const int e = base + par.tid();
        int lm = -1, st = PLP_CULL_DROP;
        if (e < hi) {
            lm = A.fresh[e];
            st = cull_state(A, lm, cur, thr);
            A.out_state[e] = (uint8_t)st;
            if (st == PLP_CULL_ERASE) ++removed;
        }
        const bool v = e < hi && st == PLP_CULL_HOLD;
        const int pos = lm_rank(par, sh.wave_n, v, n);
        if (v) A.out_fresh[lo + pos] = lm;
    }
    if (removed) par.add(sh.removed, removed);
    par.barrier();
    if (par.tid() == 0) { A.out_num_removed[r] = sh.removed; A.out_num_fresh[r] = n; }
}

// cnt given: k_cull_count over the Cv entries first; then k_cull_replay, and k_cull_dead_landmarks when an optional mask is asked for
hipError_t launch_cull_keyframes(hipStream_t st, const CullArgs& A);
hipError_t launch_cull_landmarks(hipStream_t st, const CullLmArgs& A);

}  // namespace plp
