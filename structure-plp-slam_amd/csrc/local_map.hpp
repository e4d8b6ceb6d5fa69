// module::local_map_updater (module/local_map_updater.cc:60-273) as tracking_module::update_local_map runs it (tracking_module.cc:837-906), with the
// landmarks search_local_landmarks[_line] skips because the frame holds them (:911-946): one definition for host and device (plp_local_map_* /
// plp_model_local_map_host, include/plp_front.h).  Integers only: counts, rows and order.
//
// The steps are written once over a team `P` of lanes (P::NT lanes in waves of P::WS): the kernels run them with a workgroup, the host build with a
// team of one, for which every barrier is empty, every ballot one bit and every strided loop the plain loop.  No result depends on the team's size:
// the weights are integer sums, every list position is a rank in a defined order, and the first-seen rule of the landmark lists is the minimum of
// the candidates' positions.
//
//   lm_keyframes   per frame: the weights (a table of F counters in the team's shared state), the first local key frames in ascending row with
//                  `nearest`, then the second-order walk on one wave
//   lm_mark        per (frame, local key frame): every slot's position k * cap + idx into the frame's row of the mark table by an integer minimum;
//                  the frame's own slots set a bit per landmark beside it
//   lm_compact     per frame: the candidates in order, kept iff the table holds their own position, ranked by ballot and prefix
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/plp_front.h"

namespace plp {

constexpr int kLmMaxKf = 8192;            // F: the weights of a frame are kLmMaxKf i32 counters of shared state (32 KB of the 64 KB a kernel may declare)
constexpr int kLmMaxSlots = 8192;         // cap, lcap, fcap, flcap
constexpr int kLmMaxFrames = 65535;       // B: a chunk of frames is the y extent of k_local_map_mark's grid
constexpr int kLmCovis = 10;              // get_top_n_covisibilities(10), :179
constexpr int kLmThreads = 512;           // the workgroup of k_local_map_keyframes and k_local_map_compact
constexpr int kLmMarkThreads = 256;       // the workgroup of k_local_map_mark
constexpr long long kLmDefaultWorkspace = 256ll << 20;

struct LmArgs {
    int B, F, C, L, LL, T, cap, lcap, fcap, flcap, frm_stride, frm_stride_lines, max_kf, k_cap, m_cap, ml_cap;
    int lines;                                // kf_lm_lines was given: the line side runs and its counts are written
    const uint8_t* kf_erased; const int32_t* kf_covis; const int32_t* kf_parent; const int32_t* kf_children_offsets; const int32_t* kf_children;
    const int32_t* kf_lm; const int32_t* kf_counts; const int32_t* kf_lm_lines; const int32_t* kf_kl_counts;
    const int32_t* obs_offsets; const int32_t* obs_kf; const uint8_t* lm_erased; const uint8_t* lm_erased_lines;
    const int32_t* frm_lm; const int32_t* frm_counts; const int32_t* frm_lm_lines; const int32_t* frm_kl_counts;
    uint8_t* out_status; int32_t* out_num_first; int32_t* out_num_kf; int32_t* out_local_kf; int32_t* out_first_weight; int32_t* out_nearest_kf;
    int32_t* out_num_lm; int32_t* out_local_lm; uint8_t* out_held; int32_t* out_num_lines; int32_t* out_local_lines; uint8_t* out_held_lines;
    // the chunk of frames [b0, b0 + nb) whose mark table `ws` holds: nb rows of ws_rows words, then nb rows of ws_words bitmap words
    uint32_t* ws; int b0, nb, ws_rows, ws_words;
};
__host__ __device__ __forceinline__ int lm_ws_rows(int L, int LL) { return L > LL ? L : LL; }
__host__ __device__ __forceinline__ int lm_ws_words(int L, int LL) { return (lm_ws_rows(L, LL) + 31) / 32; }
__host__ __device__ __forceinline__ size_t lm_ws_frame_bytes(int L, int LL) { return ((size_t)lm_ws_rows(L, LL) + lm_ws_words(L, LL)) * 4; }
// key-frame blocks of k_local_map_mark's grid: the local key frames are distinct rows, so there are at most F of them
__host__ __device__ __forceinline__ int lm_mark_blocks(int k_cap, int F) { return k_cap < F ? k_cap : F; }

// the point or the line side of the landmark lists
struct LmList {
    const int32_t* kf_lm; const int32_t* kf_counts; const uint8_t* erased; const int32_t* frm; const int32_t* frm_counts;
    int cap, rows, fcap, fstride, out_cap, overflow;
    int32_t* out_num; int32_t* out_list; uint8_t* out_held;
};
template <bool LINES> __host__ __device__ __forceinline__ LmList lm_list(const LmArgs& A) {
    LmList S;
    if (LINES) {
        S.kf_lm = A.kf_lm_lines; S.kf_counts = A.kf_kl_counts; S.erased = A.lm_erased_lines; S.frm = A.frm_lm_lines; S.frm_counts = A.frm_kl_counts;
        S.cap = A.lcap; S.rows = A.LL; S.fcap = A.flcap; S.fstride = A.frm_stride_lines; S.out_cap = A.ml_cap; S.overflow = PLP_LOCAL_MAP_LINE_OVERFLOW;
        S.out_num = A.out_num_lines; S.out_list = A.out_local_lines; S.out_held = A.out_held_lines;
    } else {
        S.kf_lm = A.kf_lm; S.kf_counts = A.kf_counts; S.erased = A.lm_erased; S.frm = A.frm_lm; S.frm_counts = A.frm_counts;
        S.cap = A.cap; S.rows = A.L; S.fcap = A.fcap; S.fstride = A.frm_stride; S.out_cap = A.m_cap; S.overflow = PLP_LOCAL_MAP_LM_OVERFLOW;
        S.out_num = A.out_num_lm; S.out_list = A.out_local_lm; S.out_held = A.out_held;
    }
    return S;
}

// the shared state of lm_keyframes: LDS on the device, the stack on the host
struct LmShared {
    int32_t w[kLmMaxKf];                      // keyframe_weights_t, :93
    uint32_t local[kLmMaxKf / 32];            // local_map_update_identifier == frm_id_, :130, :161-165
    unsigned long long best[kLmThreads];
    int32_t wave_n[kLmThreads / 64];
    int32_t any;
};
struct LmSharedCompact { int32_t wave_n[kLmThreads / 64]; };

// the team of one of the host build
struct LmTeamHost {
    static constexpr int NT = 1, WS = 1, NW = 1;
    __host__ __device__ int tid() const { return 0; }
    __host__ __device__ int lane() const { return 0; }
    __host__ __device__ int wave() const { return 0; }
    __host__ __device__ void barrier() const {}
    __host__ __device__ unsigned long long ballot(bool v) const { return v ? 1ull : 0ull; }
    __host__ __device__ void add(int32_t& t, int v) const { t += v; }
    __host__ __device__ void bit_or(uint32_t& t, uint32_t v) const { t |= v; }
    __host__ __device__ void min(uint32_t& t, uint32_t v) const { if (v < t) t = v; }
};

// a count cut to [0, cap]; NULL = cap
__host__ __device__ __forceinline__ int lm_count(const int32_t* counts, int row, int cap) {
    if (!counts) return cap;
    const int c = counts[row];
    return c < 0 ? 0 : c > cap ? cap : c;
}
// [lo, hi) of an offsets table, cut to [0, n]
__host__ __device__ __forceinline__ void lm_run(const int32_t* offsets, int row, int n, int& lo, int& hi) {
    lo = offsets[row]; hi = offsets[row + 1];
    lo = lo < 0 ? 0 : lo > n ? n : lo;
    hi = hi < lo ? lo : hi > n ? n : hi;
}
// a landmark row that is in its table and not erased (a slot whose landmark is erased counts as empty: tracking_module.cc:840-870, :217-224)
__host__ __device__ __forceinline__ bool lm_present(int lm, int rows, const uint8_t* erased) {
    return (unsigned)lm < (unsigned)rows && !(erased && erased[lm]);
}

// an ordered compaction step over the team: the rank of this lane's item among the flagged ones, n moves on; two barriers (local_ba.hpp's la_rank
// over a bare array of wave counts: that one is bound to LaShared)
template <class P> __host__ __device__ __forceinline__ int lm_rank(P& par, int32_t* wave_n, bool v, int& n) {
    const unsigned long long m = par.ballot(v);
    if (par.lane() == 0) wave_n[par.wave()] = (int)__builtin_popcountll(m);
    par.barrier();
    int off = n, tot = 0;
    for (int u = 0; u < P::NW; ++u) {
        if (u < par.wave()) off += wave_n[u];
        tot += wave_n[u];
    }
    n += tot;
    par.barrier();
    return off + (int)__builtin_popcountll(m & ((1ull << par.lane()) - 1ull));
}

// add_second_local_keyframe's test (:150-168) without the append
__host__ __device__ __forceinline__ bool lm_second_ok(const LmArgs& A, const LmShared& sh, int kf) {
    if ((unsigned)kf >= (unsigned)A.F) return false;                 // !keyfrm
    if (A.kf_erased && A.kf_erased[kf]) return false;                // will_be_erased()
    return !((sh.local[kf >> 5] >> (kf & 31)) & 1u);                 // local_map_update_identifier == frm_id_
}
// the first entry of list[lo, hi) that passes the test, in tiles of one wave: its row, or -1 (:180-186, :190-196)
template <class P> __host__ __device__ __forceinline__ int lm_first_ok(const LmArgs& A, const LmShared& sh, P& par, const int32_t* list, int lo, int hi) {
    for (int base = lo; base < hi; base += P::WS) {
        const int i = base + par.lane();
        const unsigned long long m = par.ballot(i < hi && lm_second_ok(A, sh, list[i]));
        if (m) return list[base + __builtin_ctzll(m)];
    }
    return -1;
}

// ---- find_local_keyframes (:75-204) of frame b
template <class P> __host__ __device__ __forceinline__ void lm_keyframes(const LmArgs& A, int b, LmShared& sh, P& par) {
    const int tid = par.tid(), F = A.F;
    for (int f = tid; f < F; f += P::NT) sh.w[f] = 0;
    for (int i = tid; i < (F + 31) / 32; i += P::NT) sh.local[i] = 0;
    if (tid == 0) sh.any = 0;
    par.barrier();
    // count_keyframe_weights (:89-108): one lane per slot of the frame walks that landmark's observations
    const int fcnt = lm_count(A.frm_counts, b, A.fcap);
    const int32_t* frm = A.frm_lm + (size_t)b * A.frm_stride;
    for (int s = tid; s < fcnt; s += P::NT) {
        const int lm = frm[s];
        if (!lm_present(lm, A.L, A.lm_erased)) continue;
        int lo, hi;
        lm_run(A.obs_offsets, lm, A.T, lo, hi);
        for (int t = lo; t < hi; ++t) {
            const int kf = A.obs_kf[t];
            if ((unsigned)kf >= (unsigned)F) continue;
            par.add(sh.w[kf], 1);
            sh.any = 1;
        }
    }
    par.barrier();
    const bool lines = A.lines != 0;
    if (!sh.any) {                                                    // keyfrm_weights.empty(), :78-81
        if (tid == 0) {
            A.out_status[b] = PLP_LOCAL_MAP_NO_KEYFRAMES;
            A.out_num_first[b] = 0; A.out_num_kf[b] = 0; A.out_nearest_kf[b] = -1; A.out_num_lm[b] = 0;
            if (lines) A.out_num_lines[b] = 0;
        }
        return;
    }
    // find_first_local_keyframes (:110-141) in ascending row; nearest: the largest weight << 32 | ~row, so the first row among equal weights
    int n = 0;
    unsigned long long best = 0;
    for (int base = 0; base < F; base += P::NT) {
        const int f = base + tid;
        const bool v = f < F && sh.w[f] > 0 && !(A.kf_erased && A.kf_erased[f]);
        const int pos = lm_rank(par, sh.wave_n, v, n);
        if (!v) continue;
        par.bit_or(sh.local[f >> 5], 1u << (f & 31));
        if (pos < A.k_cap) {
            A.out_local_kf[(size_t)b * A.k_cap + pos] = f;
            if (A.out_first_weight) A.out_first_weight[(size_t)b * A.k_cap + pos] = sh.w[f];
        }
        const unsigned long long key = ((unsigned long long)(uint32_t)sh.w[f] << 32) | (uint32_t)~(uint32_t)f;
        best = key > best ? key : best;
    }
    sh.best[tid] = best;
    par.barrier();
    if (par.wave() != 0) return;
    if (tid == 0) {
        for (int i = 1; i < P::NT; ++i) best = sh.best[i] > best ? sh.best[i] : best;
        A.out_nearest_kf[b] = best ? (int32_t)~(uint32_t)best : -1;
    }
    // find_second_local_keyframes (:143-204) on one wave: the first local key frames again in ascending row
    int ns = 0;
    bool stop = false;
    for (int base = 0; base < F && !stop; base += P::WS) {
        const int f = base + par.lane();
        unsigned long long m = par.ballot(f < F && sh.w[f] > 0 && !(A.kf_erased && A.kf_erased[f]));
        while (m && !stop) {
            const int kf = base + __builtin_ctzll(m);
            m &= m - 1;
            if ((long long)A.max_kf < (long long)n + ns) { stop = true; break; }   // :171
            for (int step = 0; step < 3; ++step) {
                int c;
                if (step == 0) c = lm_first_ok(A, sh, par, A.kf_covis + (size_t)kf * kLmCovis, 0, kLmCovis);
                else if (step == 1) {
                    int lo, hi;
                    lm_run(A.kf_children_offsets, kf, A.C, lo, hi);
                    c = lm_first_ok(A, sh, par, A.kf_children, lo, hi);
                } else {
                    c = A.kf_parent[kf];
                    if (!lm_second_ok(A, sh, c)) c = -1;
                }
                if (c < 0) continue;
                if (par.lane() == 0) {
                    sh.local[c >> 5] |= 1u << (c & 31);
                    const int pos = n + ns;
                    if (pos < A.k_cap) {
                        A.out_local_kf[(size_t)b * A.k_cap + pos] = c;
                        if (A.out_first_weight) A.out_first_weight[(size_t)b * A.k_cap + pos] = 0;
                    }
                }
                ++ns;
            }
        }
    }
    if (tid == 0) {
        const bool over = n + ns > A.k_cap;
        A.out_num_first[b] = n; A.out_num_kf[b] = n + ns;
        A.out_status[b] = over ? PLP_LOCAL_MAP_KF_OVERFLOW : PLP_LOCAL_MAP_OK;
        if (over) {
            A.out_num_lm[b] = 0;
            if (lines) A.out_num_lines[b] = 0;
        }
    }
}

// whether frame b has landmark lists: not after NO_KEYFRAMES or KF_OVERFLOW
__host__ __device__ __forceinline__ bool lm_has_lists(const LmArgs& A, int b) {
    const int st = A.out_status[b];
    return st != PLP_LOCAL_MAP_NO_KEYFRAMES && st != PLP_LOCAL_MAP_KF_OVERFLOW;
}

// ---- the marks of frame b0 + bc: block k < kb marks the slots of local key frame k, block kb the frame's own slots (kb = lm_mark_blocks)
template <bool LINES, class P> __host__ __device__ __forceinline__ void lm_mark(const LmArgs& A, int bc, int k, P& par) {
    const LmList S = lm_list<LINES>(A);
    const int b = A.b0 + bc;
    if (!lm_has_lists(A, b)) return;
    uint32_t* tab = A.ws + (size_t)bc * A.ws_rows;
    uint32_t* bits = A.ws + (size_t)A.nb * A.ws_rows + (size_t)bc * A.ws_words;
    if (k < lm_mark_blocks(A.k_cap, A.F)) {
        if (k >= A.out_num_kf[b]) return;
        const int kf = A.out_local_kf[(size_t)b * A.k_cap + k];
        const int cnt = lm_count(S.kf_counts, kf, S.cap);
        for (int idx = par.tid(); idx < cnt; idx += P::NT) {
            const int lm = S.kf_lm[(size_t)kf * S.cap + idx];
            if (lm_present(lm, S.rows, S.erased)) par.min(tab[lm], (uint32_t)k * (uint32_t)S.cap + (uint32_t)idx);
        }
    } else if (S.frm) {
        const int fcnt = lm_count(S.frm_counts, b, S.fcap);
        for (int s = par.tid(); s < fcnt; s += P::NT) {
            const int lm = S.frm[(size_t)b * S.fstride + s];
            if (lm_present(lm, S.rows, S.erased)) par.bit_or(bits[lm >> 5], 1u << (lm & 31));
        }
    }
}

// ---- find_local_landmarks[_line] (:206-273) of frame b0 + bc from the marks, with the held byte
template <bool LINES, class P> __host__ __device__ __forceinline__ void lm_compact(const LmArgs& A, int bc, LmSharedCompact& sh, P& par) {
    const LmList S = lm_list<LINES>(A);
    const int b = A.b0 + bc;
    if (!lm_has_lists(A, b)) return;
    const uint32_t* tab = A.ws + (size_t)bc * A.ws_rows;
    const uint32_t* bits = A.ws + (size_t)A.nb * A.ws_rows + (size_t)bc * A.ws_words;
    const int nk = A.out_num_kf[b];
    int n = 0;
    for (int k = 0; k < nk; ++k) {
        const int kf = A.out_local_kf[(size_t)b * A.k_cap + k];
        const int cnt = lm_count(S.kf_counts, kf, S.cap);
        for (int base = 0; base < cnt; base += P::NT) {
            const int idx = base + par.tid();
            int lm = -1;
            bool v = false;
            if (idx < cnt) {
                lm = S.kf_lm[(size_t)kf * S.cap + idx];
                v = lm_present(lm, S.rows, S.erased) && tab[lm] == (uint32_t)k * (uint32_t)S.cap + (uint32_t)idx;
            }
            const int pos = lm_rank(par, sh.wave_n, v, n);
            if (v && pos < S.out_cap) {
                S.out_list[(size_t)b * S.out_cap + pos] = lm;
                S.out_held[(size_t)b * S.out_cap + pos] = (uint8_t)((bits[lm >> 5] >> (lm & 31)) & 1u);
            }
        }
    }
    if (par.tid() == 0) {
        S.out_num[b] = n;
        if (n > S.out_cap && A.out_status[b] == PLP_LOCAL_MAP_OK) A.out_status[b] = (uint8_t)S.overflow;
    }
}

hipError_t launch_local_map_keyframes(hipStream_t st, const LmArgs& A);
// one chunk: A.ws cleared on the stream, then the marks and the compaction; lines: the line side
hipError_t launch_local_map_lists(hipStream_t st, const LmArgs& A, bool lines);

}  // namespace plp
