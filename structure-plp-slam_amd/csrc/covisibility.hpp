// data::graph_node (data/graph_node.cc:36-285): update_connections for a list of G owner key frames over one map snapshot and
// erase_all_connections for a set of key frames, with the graph kept as tables: one definition for host and device (plp_covisibility_update_* /
// plp_covisibility_erase_* / plp_model_covisibility_*_host, include/plp_front.h).  Integers only: counts, a threshold
// and one total order.
//
// The steps are written once over a team `P` of lanes, as local_map.hpp's are (its helpers and its team of one serve here too): the kernels run
// them with a workgroup, the host build with a team of one.  No result depends on the team's size or on the order in which lanes or workgroups
// arrive: the weights are integer sums, the connected rows are written by rank in ascending row, the ordered list by rank in the key below, which
// is unique, and an overlay is a pure function of the owners' base rows.
//
//   cv_count   per owner: W (a table of F counters in the team's shared state), `nearest`, the pairs, then base C and base O into the call's scratch
//   cv_apply   per key frame: the base (the owner's own, or the row as it stands) with the overlays of D21 applied; the row, the parent, the status
//   cv_erase   per key frame: a surviving row loses the erased key frames that hold it (phase 0); the erased rows end empty (phase 1)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/plp_front.h"
#include "local_map.hpp"

namespace plp {

constexpr int kCvMaxKf = kLmMaxKf;            // F: W is kCvMaxKf i32 counters of shared state, and a row is 13 bits of the key
constexpr int kCvMaxSlots = kLmMaxSlots;      // cap
constexpr int kCvThreads = 256;               // every workgroup of covisibility_kernels.hip
constexpr int kCvWeightThr = 15;              // weight_thr_ (graph_node.h)

struct CvArgs {
    int F, L, T, cap, G, conn_cap, covis_cap, phase;
    const int32_t* kf_lm; const int32_t* kf_counts; const int32_t* obs_offsets; const int32_t* obs_kf; const uint8_t* lm_erased; const uint32_t* kf_id;
    int32_t* kf_conn; int32_t* kf_conn_w; int32_t* kf_n_conn; int32_t* kf_covis; int32_t* kf_covis_w; int32_t* kf_n_covis;
    int32_t* kf_parent; uint8_t* kf_parent_unset;
    const int32_t* owners; const uint8_t* erased;
    uint8_t* out_status; int32_t* out_nearest; int32_t* out_max_weight; uint8_t* out_touched;
    // what the context owns (update only): the position of every row in `owners` ([F], -1 = not an owner; cleared before cv_count), and per
    // position the status of cv_count, nearest, the maximal weight, the true lengths of base C and base O, and their rows cut to the caps
    int32_t* pos_of; int32_t* o_state; int32_t* o_nearest; int32_t* o_maxw; int32_t* b_n_conn; int32_t* b_n_covis;
    int32_t* b_conn; int32_t* b_conn_w; int32_t* b_covis; int32_t* b_covis_w;
};

// the scratch of one update as one block of i32 that starts at A.pos_of: its length, and the other pointers into it
__host__ __device__ __forceinline__ size_t cv_scratch_words(int F, int G, int conn_cap, int covis_cap) {
    return (size_t)F + (size_t)G * (5 + 2 * ((size_t)conn_cap + (size_t)covis_cap));
}
inline void cv_scratch_split(CvArgs& A) {
    const size_t G = (size_t)A.G;
    A.o_state = A.pos_of + A.F; A.o_nearest = A.o_state + G; A.o_maxw = A.o_nearest + G; A.b_n_conn = A.o_maxw + G; A.b_n_covis = A.b_n_conn + G;
    A.b_conn = A.b_n_covis + G; A.b_conn_w = A.b_conn + G * A.conn_cap; A.b_covis = A.b_conn_w + G * A.conn_cap; A.b_covis_w = A.b_covis + G * A.covis_cap;
}

// the shared state of a team: LDS on the device, the heap on the host
struct CvShared {
    int32_t w[kCvMaxKf];                      // by row: W of cv_count, C of cv_apply (-1 = absent); by position: the weights of cv_erase
    uint16_t row[kCvMaxKf];                   // the rows of the list that cv_order ranks
    unsigned long long best[kCvThreads];
    int32_t wave_n[kCvThreads / 64];
    int32_t any, flag;
};

// ---- the definitions every build shares
// the order of ordered_covisibilities_: std::pair<unsigned, keyframe*> descending (:165, :208); rows stand in for pointers, so the key is unique
__host__ __device__ __forceinline__ unsigned long long cv_key(int32_t w, int row) { return ((unsigned long long)(uint32_t)w << 13) | (uint32_t)row; }
// weight_thr_ < weight (:145)
__host__ __device__ __forceinline__ bool cv_over(int32_t w) { return kCvWeightThr < w; }
// whether `row` with weight w is one of the owner's pairs (:145-154): above the threshold, or the one node kept when nothing is
__host__ __device__ __forceinline__ bool cv_is_pair(int32_t w, int row, int32_t max_weight, int nearest) {
    return cv_over(w) || (!cv_over(max_weight) && row == nearest);
}
// add_connection (:36-59): whether the connected map changes, and with it the ordered list
__host__ __device__ __forceinline__ bool cv_overlay_changes(int32_t held, int32_t w) { return held != w; }   // held: -1 = absent

// the position of `row` in an ascending list, or -1
__host__ __device__ __forceinline__ int cv_find(const int32_t* rows, int n, int row) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (rows[mid] < row) lo = mid + 1; else hi = mid;
    }
    return (lo < n && rows[lo] == row) ? lo : -1;
}
__host__ __device__ __forceinline__ int cv_cut(int n, int cap) { return n < 0 ? 0 : n > cap ? cap : n; }

// the n entries of sh.row (weights: sh.w by row when BY_ROW, by position otherwise) in descending key into a list of `cap` slots: the rank of an
// entry is the number of larger keys; -1 / 0 behind the last entry
template <bool BY_ROW, class P> __host__ __device__ __forceinline__ void cv_order(P& par, const CvShared& sh, int n, int32_t* rows, int32_t* weights, int cap) {
    for (int i = par.tid(); i < n; i += P::NT) {
        const int r = sh.row[i];
        const int32_t w = sh.w[BY_ROW ? r : i];
        const unsigned long long key = cv_key(w, r);
        int rank = 0;
        for (int q = 0; q < n; ++q) {
            const int rq = sh.row[q];
            rank += cv_key(sh.w[BY_ROW ? rq : q], rq) > key;
        }
        if (rank < cap) { rows[rank] = r; weights[rank] = w; }
    }
    for (int i = n + par.tid(); i < cap; i += P::NT) { rows[i] = -1; weights[i] = 0; }
}

// ---- update_connections (:92-165) of the owner at position p of the list, up to the point where it touches state
template <class P> __host__ __device__ __forceinline__ void cv_count(const CvArgs& A, int p, CvShared& sh, P& par) {
    const int tid = par.tid(), F = A.F;
    const int k = A.owners[p];
    if (tid == 0) { sh.any = 0; sh.flag = 0; }
    for (int f = tid; f < F; f += P::NT) sh.w[f] = 0;
    par.barrier();
    int code = -1;
    if ((unsigned)k >= (unsigned)F) code = PLP_COVIS_ROW_ABSENT;
    else {
        for (int q = tid; q < p; q += P::NT)
            if (A.owners[q] == k) sh.flag = 1;
        par.barrier();
        if (sh.flag) code = PLP_COVIS_DUPLICATE;
    }
    if (code < 0) {
        if (tid == 0) A.pos_of[k] = p;
        // :96-121: one lane per slot of the owner walks that landmark's observations
        const int cnt = lm_count(A.kf_counts, k, A.cap);
        for (int s = tid; s < cnt; s += P::NT) {
            const int lm = A.kf_lm[(size_t)k * A.cap + s];
            if (!lm_present(lm, A.L, A.lm_erased)) continue;
            int lo, hi;
            lm_run(A.obs_offsets, lm, A.T, lo, hi);
            for (int t = lo; t < hi; ++t) {
                const int kf = A.obs_kf[t];
                if ((unsigned)kf >= (unsigned)F || kf == k) continue;
                par.add(sh.w[kf], 1);
                sh.any = 1;
            }
        }
        par.barrier();
        if (!sh.any) code = PLP_COVIS_NO_SHARED;                          // keyfrm_weights.empty(), :123-126
    }
    if (code >= 0) {
        if (tid == 0) {
            A.o_state[p] = code; A.out_status[p] = (uint8_t)code;
            if (A.out_nearest) A.out_nearest[p] = -1;
            if (A.out_max_weight) A.out_max_weight[p] = 0;
        }
        return;
    }
    // :134-149 in ascending row: base C, the largest key (so the largest row among the maximal weights, the `<=` of :139), the pairs
    int32_t* bc = A.b_conn + (size_t)p * A.conn_cap;
    int32_t* bw = A.b_conn_w + (size_t)p * A.conn_cap;
    int n = 0, np = 0;
    unsigned long long best = 0;
    for (int base = 0; base < F; base += P::NT) {
        const int f = base + tid;
        const int32_t w = f < F ? sh.w[f] : 0;
        const int pos = lm_rank(par, sh.wave_n, w > 0, n);
        const int ppos = lm_rank(par, sh.wave_n, cv_over(w), np);
        if (w > 0) {
            if (pos < A.conn_cap) { bc[pos] = f; bw[pos] = w; }
            const unsigned long long key = cv_key(w, f);
            best = key > best ? key : best;
        }
        if (cv_over(w)) sh.row[ppos] = (uint16_t)f;
    }
    sh.best[tid] = best;
    par.barrier();
    for (int i = 0; i < P::NT; ++i) best = sh.best[i] > best ? sh.best[i] : best;
    const int nearest = (int)(best & (unsigned long long)(kCvMaxKf - 1));
    const int32_t maxw = (int32_t)(best >> 13);
    if (np == 0) {                                                        // add ONE node at least, :151-154
        if (tid == 0) sh.row[0] = (uint16_t)nearest;
        np = 1;
    }
    par.barrier();
    cv_order<true>(par, sh, np, A.b_covis + (size_t)p * A.covis_cap, A.b_covis_w + (size_t)p * A.covis_cap, A.covis_cap);
    if (tid == 0) {
        A.o_state[p] = PLP_COVIS_OK; A.o_nearest[p] = nearest; A.o_maxw[p] = maxw; A.b_n_conn[p] = n; A.b_n_covis[p] = np;
        if (A.out_nearest) A.out_nearest[p] = nearest;
        if (A.out_max_weight) A.out_max_weight[p] = maxw;
    }
}

// ---- the final state of key frame j after the whole list (D21): its base, the overlays of the owners that name it, the row
template <class P> __host__ __device__ __forceinline__ void cv_apply(const CvArgs& A, int j, CvShared& sh, P& par) {
    const int tid = par.tid(), F = A.F;
    const int pj = A.pos_of[j];
    const bool has_base = pj >= 0 && A.o_state[pj] == PLP_COVIS_OK;
    for (int f = tid; f < F; f += P::NT) sh.w[f] = -1;
    if (tid == 0) { sh.any = 0; sh.flag = 0; }
    par.barrier();
    const int32_t* src = has_base ? A.b_conn + (size_t)pj * A.conn_cap : A.kf_conn + (size_t)j * A.conn_cap;
    const int32_t* src_w = has_base ? A.b_conn_w + (size_t)pj * A.conn_cap : A.kf_conn_w + (size_t)j * A.conn_cap;
    const int n_base = has_base ? A.b_n_conn[pj] : A.kf_n_conn[j];
    const int n_src = cv_cut(n_base, A.conn_cap);
    for (int i = tid; i < n_src; i += P::NT) {
        const int r = src[i];
        if ((unsigned)r < (unsigned)F) sh.w[r] = src_w[i];
    }
    par.barrier();
    // the overlays: owner k at position p calls add_connection(j <- k, w) iff j is one of its pairs; after j's own turn only when j has a base.
    // The owners are distinct rows, so every lane writes another counter.
    for (int p = (has_base ? pj + 1 : 0) + tid; p < A.G; p += P::NT) {
        if (A.o_state[p] != PLP_COVIS_OK) continue;
        const int k = A.owners[p];
        if (k == j) continue;
        const int nk = A.b_n_conn[p], m = cv_cut(nk, A.conn_cap);
        const int32_t* rows = A.b_conn + (size_t)p * A.conn_cap;
        const int at = cv_find(rows, m, j);
        if (at < 0) {
            // the owner's row was cut at conn_cap and j lies behind the cut: whether j is a pair cannot be told
            if (nk > A.conn_cap && (m == 0 || rows[m - 1] < j)) sh.any = 1;
            continue;
        }
        const int32_t w = A.b_conn_w[(size_t)p * A.conn_cap + at];
        if (!cv_is_pair(w, j, A.o_maxw[p], A.o_nearest[p])) continue;
        if (cv_overlay_changes(sh.w[k], w)) { sh.w[k] = w; sh.flag = 1; }
    }
    par.barrier();
    const bool changed = sh.flag != 0, blind = sh.any != 0;
    if (!has_base && !changed) {
        if (tid == 0 && A.out_touched) A.out_touched[j] = blind ? 2 : 0;
        return;
    }
    // C in ascending row
    int32_t* conn = A.kf_conn + (size_t)j * A.conn_cap;
    int32_t* conn_w = A.kf_conn_w + (size_t)j * A.conn_cap;
    int n = 0;
    for (int base = 0; base < F; base += P::NT) {
        const int f = base + tid;
        const int32_t w = f < F ? sh.w[f] : -1;
        const int pos = lm_rank(par, sh.wave_n, w >= 0, n);
        if (w < 0) continue;
        if (pos < A.conn_cap) { conn[pos] = f; conn_w[pos] = w; }
        sh.row[pos] = (uint16_t)f;
    }
    for (int i = n + tid; i < A.conn_cap; i += P::NT) { conn[i] = -1; conn_w[i] = 0; }
    const int n_conn = n_base > A.conn_cap && n_base > n ? n_base : n;  // a base cut at the cap: its own length, the least the row can have
    par.barrier();
    // O: all of C once an overlay changed it (update_covisibility_orders, :195-219), the owner's thresholded list otherwise
    int32_t* covis = A.kf_covis + (size_t)j * A.covis_cap;
    int32_t* covis_w = A.kf_covis_w + (size_t)j * A.covis_cap;
    int n_covis;
    if (changed) {
        cv_order<true>(par, sh, n, covis, covis_w, A.covis_cap);
        n_covis = n_conn;
    } else {
        n_covis = A.b_n_covis[pj];
        const int m = cv_cut(n_covis, A.covis_cap);
        for (int i = tid; i < A.covis_cap; i += P::NT) {
            covis[i] = i < m ? A.b_covis[(size_t)pj * A.covis_cap + i] : -1;
            covis_w[i] = i < m ? A.b_covis_w[(size_t)pj * A.covis_cap + i] : 0;
        }
    }
    if (tid != 0) return;
    A.kf_n_conn[j] = n_conn; A.kf_n_covis[j] = n_covis;
    if (has_base && A.kf_parent_unset[j] && A.kf_id[j] != 0u) {          // :184-191
        A.kf_parent[j] = A.o_nearest[pj];
        A.kf_parent_unset[j] = 0;
    }
    const bool over = n_conn > A.conn_cap || n_covis > A.covis_cap || blind;
    if (A.out_touched) A.out_touched[j] = over ? 2 : 1;
    if (has_base) A.out_status[pj] = (uint8_t)(over ? PLP_COVIS_OVERFLOW : PLP_COVIS_OK);
}

// ---- erase_all_connections (:79-90) of every row of A.erased, for key frame j.  Phase 0 writes the surviving rows and reads the erased ones;
// phase 1 empties the erased rows
template <class P> __host__ __device__ __forceinline__ void cv_erase(const CvArgs& A, int j, CvShared& sh, P& par) {
    const int tid = par.tid(), F = A.F;
    int32_t* conn = A.kf_conn + (size_t)j * A.conn_cap;
    int32_t* conn_w = A.kf_conn_w + (size_t)j * A.conn_cap;
    int32_t* covis = A.kf_covis + (size_t)j * A.covis_cap;
    int32_t* covis_w = A.kf_covis_w + (size_t)j * A.covis_cap;
    const bool gone = A.erased[j] != 0;
    if (A.phase == 1) {
        if (!gone) return;
        for (int i = tid; i < A.conn_cap; i += P::NT) { conn[i] = -1; conn_w[i] = 0; }
        for (int i = tid; i < A.covis_cap; i += P::NT) { covis[i] = -1; covis_w[i] = 0; }
        if (tid == 0) {
            A.kf_n_conn[j] = 0; A.kf_n_covis[j] = 0; A.out_status[j] = PLP_COVIS_OK;
            if (A.out_touched) A.out_touched[j] = 1;
        }
        return;
    }
    if (gone) return;
    if (tid == 0) sh.flag = 0;
    par.barrier();
    // erase_connection (:61-77) from every erased k with j in C_k (the key frames of C_k are the ones k visits) and k in C_j
    const int n0 = cv_cut(A.kf_n_conn[j], A.conn_cap);
    int n = 0;
    for (int base = 0; base < n0; base += P::NT) {
        const int i = base + tid;
        int r = -1;
        int32_t w = 0;
        bool keep = false;
        if (i < n0) {
            r = conn[i]; w = conn_w[i];
            keep = (unsigned)r < (unsigned)F;                             // a row outside the table counts as absent
            if (keep && A.erased[r]) keep = cv_find(A.kf_conn + (size_t)r * A.conn_cap, cv_cut(A.kf_n_conn[r], A.conn_cap), j) < 0;
            if (!keep) sh.flag = 1;
        }
        const int pos = lm_rank(par, sh.wave_n, keep, n);
        if (keep) { sh.row[pos] = (uint16_t)r; sh.w[pos] = w; }
    }
    par.barrier();
    if (!sh.flag) {
        if (tid == 0) {
            A.out_status[j] = PLP_COVIS_OK;
            if (A.out_touched) A.out_touched[j] = 0;
        }
        return;
    }
    for (int i = tid; i < A.conn_cap; i += P::NT) {
        conn[i] = i < n ? (int32_t)sh.row[i] : -1;
        conn_w[i] = i < n ? sh.w[i] : 0;
    }
    cv_order<false>(par, sh, n, covis, covis_w, A.covis_cap);
    if (tid == 0) {
        const bool over = n > A.covis_cap;
        A.kf_n_conn[j] = n; A.kf_n_covis[j] = n;
        A.out_status[j] = (uint8_t)(over ? PLP_COVIS_OVERFLOW : PLP_COVIS_OK);
        if (A.out_touched) A.out_touched[j] = over ? 2 : 1;
    }
}

// pos_of cleared on the stream, then k_covis_count (a workgroup per owner) and k_covis_apply (a workgroup per key frame)
hipError_t launch_covisibility_update(hipStream_t st, const CvArgs& A);
// k_covis_erase twice (a workgroup per key frame): phase 0, phase 1
hipError_t launch_covisibility_erase(hipStream_t st, CvArgs A);

}  // namespace plp
