// K4  key-point distribution (quadtree) on the GPU: one 256-thread workgroup per (level, frame).
//
// Restates distribute_keypoints_via_tree (reference src/PLPSLAM/feature/orb_extractor.cc:468-685)
// in the sort-based form proven equivalent on the host in quadtree_model.hpp:
//   1. gather the level's per-cell candidate lists in reference order (cell row, cell col, row-major)
//   2. one tree key per candidate (initial node + 2 bits per split), stable sort by key: by rank inside LDS for levels of at most kQtSmallN
//      candidates (which never touch the HBM scratch), LSD radix sort over the scratch for larger ones
//   3. every node = a range of the sorted array; whole-list split passes and the "fullest first"
//      fill phase run data-parallel over node records with prefix sums giving the list order
//   4. per node: maximum score, ties to the smallest candidate index
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>

#include "orb_device.hpp"
#include "plp_barrier.hpp"
#include "plp_common.hpp"
#include "quadtree_model.hpp"

namespace plp {

constexpr int kQtMaxNodes = kQtMaxNodesLds;   // hard upper bound of the node arrays: what 160 KB of LDS hold (orb_device.hpp; 3 * quota + 8 nodes: quota up to 1960 per level)
// One block of LDS serves as the cell prefix (n_cells words), then the radix counters [16 digits][segments] (u16) of levels of up to blk_words / 8 wave-sized
// segments, then the sorted-key cache (blk_words keys); larger levels use the HBM scratch.  blk_words = 2048 (8 KB: 256 segments = 16384 candidates in LDS) -- or 1024
// for a per-level quota above 1960 (round 6: the 4 KB that buys fit the node arrays of one level at K = 2000, the reference's single-level configuration).
constexpr int kQtBlkWords = 2048, kQtBlkWordsSmall = 1024;
// Levels of at most kQtSmallN candidates (every level of a 640 x 480 frame at K = 1000: 126 - 440) are gathered by element, sorted by RANK in LDS and selected from LDS:
// no pass over the HBM scratch, one barrier for the sort (profiles/r24_quadtree.md).  While it sorts, a level keeps three words per candidate (sort key, full key, packed
// candidate) in the space of the node arrays, which are idle until the initial nodes are written -- at least 256 * 26 bytes of them -- and afterwards ten bytes per
// candidate (sorted key, packed candidate, u16 index) in the 4 * blk_words bytes of the block: qt_small_limit().
#if defined(PLP_QT_PROF) && defined(PLP_QT_PROF_SMALL_N)
constexpr int kQtSmallN = PLP_QT_PROF_SMALL_N;   // the diagnostic build only: 0 sends every level down the large path
#else
constexpr int kQtSmallN = 512;
#endif
static_assert(kQtSmallN % 4 == 0 && 3 * 4 * kQtSmallN <= 256 * 26, "the rank sort's three arrays alias the node arrays of the smallest max_nodes (256)");
__host__ __device__ constexpr int qt_small_limit(int blk_words) { return 2 * blk_words / 5 < kQtSmallN ? 2 * blk_words / 5 : kQtSmallN; }

// LDS of one workgroup, carved from dynamic shared memory: the node arrays are sized by the largest per-level quota
// (a list never holds more than 3 * quota + 3 nodes), so that 2-3 workgroups fit a CU for the usual K = 1000..2000
// (a fixed 85 KB layout had left one workgroup = four waves per CU).
struct QtShared {
    uint16_t* cnt;                  // [16 * kQtSegLds] radix counters [digit][segment]      } one 8 KB block
    uint32_t* big;                  // [kQtKeyCache] cell prefix, later the sorted-key cache  }
    // node records, two generations (ping-pong): start / end of the node's range, depth, leaf flag.  Addressed by arithmetic:
    // arrays of pointers indexed by the generation had put the whole struct into scratch memory.
    uint16_t* ns0;                  // ns(0), ne(0), ns(1), ne(1): max_nodes entries each
    uint8_t* nd0;                   // nd(0), nleaf(0), nd(1), nleaf(1): max_nodes bytes each
    __device__ __forceinline__ uint16_t* ns(int k) const { return ns0 + (size_t)k * 2 * max_nodes; }
    __device__ __forceinline__ uint16_t* ne(int k) const { return ns0 + (size_t)k * 2 * max_nodes + max_nodes; }
    __device__ __forceinline__ uint8_t* nd(int k) const { return nd0 + (size_t)k * 2 * max_nodes; }
    __device__ __forceinline__ uint8_t* nleaf(int k) const { return nd0 + (size_t)k * 2 * max_nodes + max_nodes; }
    uint16_t *b1, *b2, *b3;
    uint32_t* pk;                   // packed per-entry counts -> exclusive prefixes (lo16 created, hi16 kept)
    uint16_t *pool_pos, *pool_sorted;
    uint32_t* partial;
    int* misc;
    int max_nodes;
};
__host__ __device__ inline size_t qt_lds_bytes(int max_nodes, int blk_words) {
    return 4 * (size_t)blk_words + (size_t)max_nodes * (4 * 2 + 4 * 1 + 3 * 2 + 4 + 2 * 2) + 16 + 32;
}
__device__ __forceinline__ QtShared qt_carve(uint8_t* base, int mn, int blk_words) {
    QtShared S;
    S.cnt = reinterpret_cast<uint16_t*>(base); S.big = reinterpret_cast<uint32_t*>(base);
    uint8_t* p = base + 4 * (size_t)blk_words;
    S.pk = reinterpret_cast<uint32_t*>(p); p += 4 * (size_t)mn;
    S.partial = reinterpret_cast<uint32_t*>(p); p += 16;
    S.misc = reinterpret_cast<int*>(p); p += 32;
    S.ns0 = reinterpret_cast<uint16_t*>(p); p += 4 * 2 * (size_t)mn;
    S.b1 = reinterpret_cast<uint16_t*>(p); p += 2 * (size_t)mn; S.b2 = reinterpret_cast<uint16_t*>(p); p += 2 * (size_t)mn;
    S.b3 = reinterpret_cast<uint16_t*>(p); p += 2 * (size_t)mn;
    S.pool_pos = reinterpret_cast<uint16_t*>(p); p += 2 * (size_t)mn; S.pool_sorted = reinterpret_cast<uint16_t*>(p); p += 2 * (size_t)mn;
    S.nd0 = p; p += 4 * (size_t)mn;
    S.max_nodes = mn;
    return S;
}

// in-place exclusive scan of a[0..M) by the whole workgroup; returns the total.  Per-thread chunk sums are scanned
// inside each wave with shuffles; only the four wave totals cross a barrier (the kernel runs ~50 of these scans per
// level, and a 16-barrier Hillis-Steele over 256 partials had made barriers its main cost).
// An array that lives in LDS or in HBM, decided per level (wave-uniform): every access is a DS or a GLOBAL instruction behind a scalar branch -- never a FLAT one (a
// pointer chosen at run time, `n <= cap ? lds : hbm`, had made every access FLAT: round 6) -- and the code around it exists once (inlining the radix
// passes and the division once per place cost 0.1 ms per step: 83 spilled SGPRs, twice the code; `git show 09a8f08:tools/sessions/r06/run38.sh`).
template <typename T> struct DualArr {
    __attribute__((address_space(3))) T* l; T* g; bool in_lds;
    __device__ __forceinline__ T operator[](int i) const { T v; if (in_lds) v = l[i]; else v = g[i]; return v; }
    __device__ __forceinline__ void set(int i, T v) const { if (in_lds) l[i] = v; else g[i] = v; }
};
template <typename T> __device__ __forceinline__ DualArr<T> dual_arr(T* lds_ptr, T* hbm_ptr, bool in_lds) {
    return DualArr<T>{(__attribute__((address_space(3))) T*)lds_ptr, hbm_ptr, in_lds};
}
struct PtrArr32 { uint32_t* p; __device__ __forceinline__ uint32_t operator[](int i) const { return p[i]; } __device__ __forceinline__ void set(int i, uint32_t v) const { p[i] = v; } };

template <typename T, class Arr>
__device__ uint32_t block_scan_excl_arr(const Arr& a, int M, uint32_t* partial) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int chunk = (M + 255) >> 8;
    const int lo = min(tid * chunk, M), hi = min(lo + chunk, M);
    uint32_t sum = 0;
    for (int i = lo; i < hi; ++i) sum += a[i];
    uint32_t inc = sum;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t t = __shfl_up(inc, off);
        if (lane >= off) inc += t;
    }
    if (lane == 63) partial[wv] = inc;
    wg_barrier();
    const uint32_t w0 = partial[0], w1 = partial[1], w2 = partial[2], w3 = partial[3];
    const uint32_t base = (wv > 0 ? w0 : 0) + (wv > 1 ? w1 : 0) + (wv > 2 ? w2 : 0);
    uint32_t run = base + inc - sum;
    for (int i = lo; i < hi; ++i) { const uint32_t v = a[i]; a.set(i, (T)run); run += v; }
    wg_barrier();
    return w0 + w1 + w2 + w3;
}

template <typename T>
__device__ uint32_t block_scan_excl(T* a, int M, uint32_t* partial) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int chunk = (M + 255) >> 8;
    const int lo = min(tid * chunk, M), hi = min(lo + chunk, M);
    uint32_t sum = 0;
    for (int i = lo; i < hi; ++i) sum += a[i];
    uint32_t inc = sum;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t t = __shfl_up(inc, off);
        if (lane >= off) inc += t;
    }
    if (lane == 63) partial[wv] = inc;
    wg_barrier();
    const uint32_t w0 = partial[0], w1 = partial[1], w2 = partial[2], w3 = partial[3];
    const uint32_t base = (wv > 0 ? w0 : 0) + (wv > 1 ? w1 : 0) + (wv > 2 ? w2 : 0);
    uint32_t run = base + inc - sum;
    for (int i = lo; i < hi; ++i) { const uint32_t v = a[i]; a[i] = (T)run; run += v; }
    wg_barrier();
    return w0 + w1 + w2 + w3;
}

__device__ __forceinline__ uint32_t dev_qt_key(int x, int y, const LevelDev& L) {
    const unsigned ix = (unsigned)((double)(float)x / L.delta_x);
    const unsigned iy = (unsigned)((double)(float)y / L.delta_y);
    const unsigned node = ix + iy * (unsigned)L.n_init_x;
    int bx = (int)(L.delta_x * ix), ex = (int)(L.delta_x * (ix + 1));
    int by = (int)(L.delta_y * iy), ey = (int)(L.delta_y * (iy + 1));
    uint32_t key = node;
#pragma unroll
    for (int d = 0; d < kQtDepth; ++d) {
        const int mx = bx + ((ex - bx + 1) >> 1), my = by + ((ey - by + 1) >> 1);
        const unsigned xb = mx <= x, yb = my <= y;
        bx = xb ? mx : bx; ex = xb ? ex : mx;
        by = yb ? my : by; ey = yb ? ey : my;
        key = (key << 2) | (xb | (yb << 1));
    }
    return key;
}

// split node [s,e) at `depth`: boundaries of digit values 1,2,3; returns number of non-empty children
template <class KeyArr> __device__ __forceinline__ int dev_split(const KeyArr& K, int s, int e, int depth, int& o1, int& o2, int& o3) {
    if (depth >= kQtDepth) { o1 = o2 = o3 = e; return 1; }
    const int sh = 2 * (kQtDepth - 1 - depth);
    if (e - s == 1) {
        const unsigned d = (K[s] >> sh) & 3u;
        o1 = d >= 1 ? s : e; o2 = d >= 2 ? s : e; o3 = d >= 3 ? s : e;
        return 1;
    }
    int b[3];
#pragma unroll
    for (unsigned v = 1; v <= 3; ++v) {
        int lo = s, hi = e;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (((K[mid] >> sh) & 3u) >= v) hi = mid; else lo = mid + 1;
        }
        b[v - 1] = lo;
    }
    o1 = b[0]; o2 = b[1]; o3 = b[2];
    return (o1 > s) + (o2 > o1) + (o3 > o2) + (e > o3);
}

// Phase clocks of a diagnostic build (-DPLP_QT_PROF, tools/quadtree_phases.py; never the shipped library): thread 0 of every workgroup adds its shader-clock
// ticks per phase {gather, sort, sorted-key copy, initial nodes, phase 1, phase 2, selection} to its level's row of g_qt_prof, then the number of workgroups, of
// candidates, of phase-1 and phase-2 passes, the largest population of a final node (a maximum), the final nodes and the workgroups that took the small path.
#ifdef PLP_QT_PROF
__device__ unsigned long long g_qt_prof[kMaxLevels][16];
#define QT_PROF_TICK(k) (qt_t[k] = clock64())
#define QT_PROF_COUNT(v) (++v)
#define QT_PROF_REPORT()                                                                                                  \
    do {                                                                                                                  \
        if (tid == 0) {                                                                                                   \
            int pop = 0;                                                                                                  \
            for (int i = 0; i < m_out; ++i) pop = max(pop, (int)S.ne(cur)[i] - (int)S.ns(cur)[i]);                        \
            unsigned long long* P = g_qt_prof[level];                                                                     \
            for (int k = 0; k < 7; ++k) atomicAdd(&P[k], (unsigned long long)(qt_t[k + 1] - qt_t[k]));                    \
            atomicAdd(&P[7], 1ull); atomicAdd(&P[8], (unsigned long long)n); atomicAdd(&P[9], (unsigned long long)qt_np1); \
            atomicAdd(&P[10], (unsigned long long)qt_np2); atomicMax(&P[11], (unsigned long long)pop);                    \
            atomicAdd(&P[12], (unsigned long long)m); atomicAdd(&P[13], (unsigned long long)small);                       \
        }                                                                                                                 \
    } while (0)
extern "C" int plp_debug_quadtree_phases(unsigned long long* out, int reset) {
    if (out && hipMemcpyFromSymbol(out, HIP_SYMBOL(g_qt_prof), sizeof(g_qt_prof)) != hipSuccess) return 1;
    if (reset) { static const unsigned long long zero[kMaxLevels][16] = {}; if (hipMemcpyToSymbol(HIP_SYMBOL(g_qt_prof), zero, sizeof(zero)) != hipSuccess) return 1; }
    return 0;
}
#else
#define QT_PROF_TICK(k) ((void)0)
#define QT_PROF_COUNT(v) ((void)0)
#define QT_PROF_REPORT() ((void)0)
#endif

__global__ __launch_bounds__(256) void k_quadtree(const LevelDev* __restrict__ lv, int n_cells_total,
                                                  const uint32_t* __restrict__ cell_cand, const int32_t* __restrict__ cell_count,
                                                  int32_t* __restrict__ sel, int32_t* __restrict__ sel_count, int total_sel_cap,
                                                  uint8_t* __restrict__ scratch, size_t scratch_frame_stride,
                                                  int32_t* __restrict__ status, int max_nodes, int blk_words) {
    extern __shared__ __attribute__((aligned(16))) uint8_t qt_smem[];
    const QtShared S = qt_carve(qt_smem, max_nodes, blk_words);
    const int kQtSegLds = blk_words >> 3, kQtKeyCache = blk_words;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int level = blockIdx.x, frame = blockIdx.y;
    const LevelDev L = lv[level];
    const int N = L.quota;
#ifdef PLP_QT_PROF
    long long qt_t[8];
    int qt_np1 = 0, qt_np2 = 0;
#endif
    QT_PROF_TICK(0);
    uint32_t* cand = reinterpret_cast<uint32_t*>(scratch + (size_t)frame * scratch_frame_stride + L.qt_off);
    uint32_t* key = cand + L.qt_cap;
    uint32_t* idxA = key + L.qt_cap;
    uint32_t* idxB = idxA + L.qt_cap;
    uint16_t* cnt_hbm = reinterpret_cast<uint16_t*>(idxB + L.qt_cap);   // radix counters of levels with more than 32768 candidates
    int32_t* out_sel = sel + (size_t)frame * total_sel_cap + L.sel_base;
    int32_t* out_cnt = sel_count + frame * kMaxLevels + level;

    // ---- 1. gather candidates in reference order + keys
    const int32_t* cc = cell_count + (size_t)frame * n_cells_total + L.cell_base;
    for (int c = tid; c < L.n_cells; c += 256) S.big[c] = (uint32_t)cc[c];
    wg_barrier();
    int n = __builtin_amdgcn_readfirstlane((int)block_scan_excl(S.big, L.n_cells, S.partial));
    if (n > L.qt_cap) { if (tid == 0) atomicOr(status, 2); n = L.qt_cap; }
    if (n == 0) { if (tid == 0) *out_cnt = 0; return; }
    // one scalar branch per workgroup: the small path keeps the level in LDS from here on and never touches cand / key / idxA / idxB
    const bool small = n <= qt_small_limit(blk_words);
    uint32_t* const spk = S.big + n;                                  // small path: packed candidates in key order ...
    uint16_t* const sid = reinterpret_cast<uint16_t*>(S.big + 2 * n);   // ... and their indices in reference order, behind the sorted keys S.big[0, n)
    uint32_t* src = idxA;
    uint32_t* dst = idxB;
    if (small) {
        // by element: the candidate's cell from the LDS prefix (the last cell whose prefix is <= i), then ONE global load
        uint32_t* const uk = S.pk;            // key >> sort_lo, what the radix passes compare; padded to a multiple of four with 0xffffffff
        uint32_t* const fk = uk + kQtSmallN;  // full keys
        uint32_t* const upk = fk + kQtSmallN; // packed candidates
        for (int i = tid; i < n; i += 256) {
            int lo = 0, hi = L.n_cells;
            while (lo < hi) { const int mid = (lo + hi) >> 1; if (S.big[mid] <= (uint32_t)i) lo = mid + 1; else hi = mid; }
            const int c = lo - 1;
            const uint32_t pk = cell_cand[((size_t)frame * n_cells_total + L.cell_base + c) * kCellCap + ((uint32_t)i - S.big[c])];
            const uint32_t k = dev_qt_key((int)(pk & 0xfff), (int)((pk >> 12) & 0xfff), L);
            uk[i] = k >> L.sort_lo; fk[i] = k; upk[i] = pk;
        }
        if (tid < 4 && n + tid < ((n + 3) & ~3)) uk[n + tid] = 0xffffffffu;
        wg_barrier();
        QT_PROF_TICK(1);
        // ---- 2s. sort by rank (qt_rank, quadtree_model.hpp): the stable order the radix passes produce, from broadcast reads of all keys, four per ds_read_b128
        const int n4 = (n + 3) & ~3;
        const auto load4 = [uk](int j) { const uint4 q = *reinterpret_cast<const uint4*>(uk + j); return QtKey4{q.x, q.y, q.z, q.w}; };
        for (int i0 = __builtin_amdgcn_readfirstlane(wv) * 64; i0 < n; i0 += 256) {
            const int i = i0 + lane;
            const uint32_t rank = qt_rank(load4, n4, i0, i, uk[min(i, n - 1)]);
            if (i < n) { S.big[rank] = fk[i]; spk[rank] = upk[i]; sid[rank] = (uint16_t)i; }   // the block's cell prefix is dead: every wave is past the gather's barrier
        }
        QT_PROF_TICK(2);
    } else {
        // one wave per cell, through the HBM scratch
        for (int c = wv; c < L.n_cells; c += 4) {
            const int base = (int)S.big[c], cnt = cc[c];
            const uint32_t* cell = cell_cand + ((size_t)frame * n_cells_total + L.cell_base + c) * kCellCap;
            for (int j = lane; j < cnt; j += 64) {
                const int at = base + j;
                if (at < n) {
                    const uint32_t pk = cell[j];
                    cand[at] = pk;
                    key[at] = dev_qt_key((int)(pk & 0xfff), (int)((pk >> 12) & 0xfff), L);
                }
            }
        }
        wg_barrier();
        QT_PROF_TICK(1);

        // ---- 2. LSD radix sort (4 bits per pass) of candidate indices by key bits [sort_lo, sort_hi)
        const int nseg = (n + 63) >> 6;
        bool first = true;
        // The radix counters live in LDS, or -- levels with more than blk_words / 8 segments -- in HBM: a DualArr (DS or GLOBAL instructions behind a scalar branch)
        const DualArr<uint16_t> CNT = dual_arr(S.cnt, cnt_hbm, nseg <= kQtSegLds);
        for (int shift = L.sort_lo; shift < L.sort_hi; shift += 4) {
            for (int seg = wv; seg < nseg; seg += 4) {
                const int i = seg * 64 + lane;
                unsigned d = 16;
                if (i < n) d = (key[first ? (uint32_t)i : src[i]] >> shift) & 15u;
                uint32_t mine = 0;
#pragma unroll
                for (unsigned v = 0; v < 16; ++v) {
                    const unsigned long long bal = __ballot(d == v);
                    if ((unsigned)lane == v) mine = (uint32_t)__popcll(bal);
                }
                if (lane < 16) CNT.set(lane * nseg + seg, (uint16_t)mine);
            }
            wg_barrier();
            block_scan_excl_arr<uint16_t>(CNT, 16 * nseg, S.partial);
            for (int seg = wv; seg < nseg; seg += 4) {
                const int i = seg * 64 + lane;
                unsigned d = 16;
                uint32_t id = 0;
                if (i < n) { id = first ? (uint32_t)i : src[i]; d = (key[id] >> shift) & 15u; }
                // the lanes holding the same digit as this one (d = 16: the lanes past the end), from one ballot per BIT of d; selecting the
                // lane's own of sixteen per-value ballots had cost 30 registers for their copies (the kernel's register peak)
                unsigned long long mybal = ~0ull;
#pragma unroll
                for (unsigned bit = 0; bit < 5; ++bit) {
                    const bool one = (d >> bit) & 1u;
                    const unsigned long long bal = __ballot(one);
                    mybal &= one ? bal : ~bal;
                }
                if (i < n) dst[(uint32_t)CNT[d * nseg + seg] + (uint32_t)__popcll(mybal & ((1ull << lane) - 1ull))] = id;
            }
            wg_barrier();
            uint32_t* t = src; src = dst; dst = t;
            first = false;
        }
        QT_PROF_TICK(2);
        // src now holds candidate indices in key order (identity if no pass ran); dst <- sorted keys
        for (int i = tid; i < n; i += 256) {
            const uint32_t id = first ? (uint32_t)i : src[i];
            if (first) src[i] = id;
            const uint32_t k = key[id];
            dst[i] = k;
            if (n <= kQtKeyCache) S.big[i] = k;
        }
    }
    wg_barrier();
    QT_PROF_TICK(3);
    const uint32_t* sidx = src;
    // The sorted keys are read from their LDS copy when it exists, from the HBM scratch otherwise: a DualArr again
    const DualArr<uint32_t> K = dual_arr(S.big, dst, n <= kQtKeyCache);

    // ---- 3a. initial nodes = runs of equal initial-node index
    int cur = 0;
    if (tid == 0) {
        int m = 0, s = 0;
        while (s < n) {   // at most n_init (<= 8) runs; binary search each end
            const uint32_t node = K[s] >> (2 * kQtDepth);
            int lo = s, hi = n;
            while (lo < hi) { const int mid = (lo + hi) >> 1; if ((K[mid] >> (2 * kQtDepth)) > node) hi = mid; else lo = mid + 1; }
            S.ns(0)[m] = (uint16_t)s; S.ne(0)[m] = (uint16_t)lo; S.nd(0)[m] = 0; S.nleaf(0)[m] = (lo - s == 1);
            ++m; s = lo;
        }
        S.misc[0] = m; S.misc[1] = 0; S.misc[3] = 0;
    }
    wg_barrier();
    QT_PROF_TICK(4);
    int m = S.misc[0];
    bool filled = false, failed = false;

    // ---- 3b. phase 1: split every non-leaf entry, children to the front in reverse creation order.  The pool size (children with more than one point) is counted
    // in misc[1] and misc[3] by turns: a pass resets the NEXT pass's counter behind its first barrier -- every thread has read that counter's last value before it got
    // there, and three more barriers follow before the next pass adds to it -- so neither the reset nor the end of the loop needs a barrier of its own
    int pslot = 1;
    while (true) {
        QT_PROF_COUNT(qt_np1);
        const int prev = m;
        for (int i = tid; i < m; i += 256) {
            if (S.nleaf(cur)[i]) { S.pk[i] = 1u << 16; continue; }
            int o1, o2, o3;
            const int s = S.ns(cur)[i], e = S.ne(cur)[i];
            const int k = dev_split(K, s, e, S.nd(cur)[i], o1, o2, o3);
            S.b1[i] = (uint16_t)o1; S.b2[i] = (uint16_t)o2; S.b3[i] = (uint16_t)o3;
            S.pk[i] = (uint32_t)k;
            const int big = (o1 - s > 1) + (o2 - o1 > 1) + (o3 - o2 > 1) + (e - o3 > 1);
            if (big) atomicAdd(&S.misc[pslot], big);
        }
        wg_barrier();
        if (tid == 0) S.misc[pslot ^ 2] = 0;
        const uint32_t tot = block_scan_excl(S.pk, m, S.partial);
        const int T = (int)(tot & 0xffff), kept = (int)(tot >> 16);
        const int m_new = T + kept;
        if (m_new > S.max_nodes) { failed = true; break; }
        const int nxt = cur ^ 1;
        for (int i = tid; i < m; i += 256) {
            const uint32_t p = S.pk[i];
            const int s = S.ns(cur)[i], e = S.ne(cur)[i];
            if (S.nleaf(cur)[i]) {
                const int pos = T + (int)(p >> 16);
                S.ns(nxt)[pos] = (uint16_t)s; S.ne(nxt)[pos] = (uint16_t)e; S.nd(nxt)[pos] = S.nd(cur)[i]; S.nleaf(nxt)[pos] = 1;
                continue;
            }
            int q = (int)(p & 0xffff);
            const int b[5] = {s, S.b1[i], S.b2[i], S.b3[i], e};
            const uint8_t dep = (uint8_t)min((int)S.nd(cur)[i] + 1, 255);
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (b[c + 1] > b[c]) {
                    const int pos = T - 1 - q;
                    S.ns(nxt)[pos] = (uint16_t)b[c]; S.ne(nxt)[pos] = (uint16_t)b[c + 1]; S.nd(nxt)[pos] = dep; S.nleaf(nxt)[pos] = 0;
                    ++q;
                }
        }
        wg_barrier();
        cur = nxt; m = m_new;
        const int pool = S.misc[pslot];
        pslot ^= 2;
        if (N <= m || m == prev) { filled = true; break; }
        if (N < m + pool) break;
    }

    // ---- 3c. phase 2: split the fullest entries first until the quota is reached
    QT_PROF_TICK(5);
    while (!filled && !failed) {
        QT_PROF_COUNT(qt_np2);
        const int prev = m;
        // pool = entries with more than one point, in list order (ordered compaction)
        for (int i = tid; i < m; i += 256) S.pk[i] = (uint32_t)(S.ne(cur)[i] - S.ns(cur)[i] > 1);
        wg_barrier();
        const int p = __builtin_amdgcn_readfirstlane((int)block_scan_excl(S.pk, m, S.partial));
        // ... with each pool entry's order key beside it (b1 and b2, one u32 array while no split is pending): the ranking below reads ONE broadcast word per
        // comparison instead of pool_pos -> ne, ns
        uint32_t* const pkey = reinterpret_cast<uint32_t*>(S.b1);
        for (int i = tid; i < m; i += 256) {
            const int cnt = S.ne(cur)[i] - S.ns(cur)[i];
            if (cnt > 1) { const uint32_t a = S.pk[i]; S.pool_pos[a] = (uint16_t)i; pkey[a] = ((uint32_t)cnt << 12) | (uint32_t)(4095 - min(i, 4095)); }
        }
        wg_barrier();
        if (p == 0) break;   // nothing left to split
        // order: count descending, then list position ascending (== creation descending)
        for (int a = tid; a < p; a += 256) {
            const uint32_t ka = pkey[a];
            int rank = 0;
            for (int b = 0; b < p; ++b) rank += pkey[b] > ka;
            S.pool_sorted[rank] = S.pool_pos[a];
        }
        wg_barrier();
        // split in sorted order; inclusive gain prefix decides where the quota is met
        for (int j = tid; j < p; j += 256) {
            const int i = S.pool_sorted[j];
            int o1, o2, o3;
            const int k = dev_split(K, S.ns(cur)[i], S.ne(cur)[i], S.nd(cur)[i], o1, o2, o3);
            S.b1[j] = (uint16_t)o1; S.b2[j] = (uint16_t)o2; S.b3[j] = (uint16_t)o3;
            S.pk[j] = (uint32_t)k;
        }
        if (tid == 0) S.misc[2] = p;   // r+1 = number of pool entries actually split
        wg_barrier();
        block_scan_excl(S.pk, p, S.partial);   // exclusive prefix of k over sorted order
        for (int j = tid; j < p; j += 256) {
            const int i = S.pool_sorted[j];
            int k = 1;
            {   // recover k_j from the boundaries
                const int s = S.ns(cur)[i], e = S.ne(cur)[i];
                k = (S.b1[j] > s) + (S.b2[j] > S.b1[j]) + (S.b3[j] > S.b2[j]) + (e > S.b3[j]);
            }
            const int size_after = m + (int)S.pk[j] + k - (j + 1);   // m + sum_{t<=j} (k_t - 1)
            if (N <= size_after) atomicMin(&S.misc[2], j + 1);
        }
        wg_barrier();
        const int nsplit = S.misc[2];
        // total children created by the first nsplit entries
        int T;
        {
            const int jl = nsplit - 1, il = S.pool_sorted[jl];
            const int s = S.ns(cur)[il], e = S.ne(cur)[il];
            const int kl = (S.b1[jl] > s) + (S.b2[jl] > S.b1[jl]) + (S.b3[jl] > S.b2[jl]) + (e > S.b3[jl]);
            T = (int)S.pk[jl] + kl;
        }
        const int m_new = T + m - nsplit;
        if (m_new > S.max_nodes) { failed = true; break; }
        const int nxt = cur ^ 1;
        // erased flags + survivors' new positions
        wg_barrier();
        for (int j = tid; j < nsplit; j += 256) {
            const int i = S.pool_sorted[j];
            int q = (int)S.pk[j];
            const int s = S.ns(cur)[i], e = S.ne(cur)[i];
            const int b[5] = {s, S.b1[j], S.b2[j], S.b3[j], e};
            const uint8_t dep = (uint8_t)min((int)S.nd(cur)[i] + 1, 255);
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (b[c + 1] > b[c]) {
                    const int pos = T - 1 - q;
                    S.ns(nxt)[pos] = (uint16_t)b[c]; S.ne(nxt)[pos] = (uint16_t)b[c + 1]; S.nd(nxt)[pos] = dep; S.nleaf(nxt)[pos] = 0;
                    ++q;
                }
            S.nleaf(cur)[i] |= 2;   // mark erased
        }
        wg_barrier();
        for (int i = tid; i < m; i += 256) S.pk[i] = (S.nleaf(cur)[i] & 2) ? 0u : 1u;
        wg_barrier();
        block_scan_excl(S.pk, m, S.partial);
        for (int i = tid; i < m; i += 256)
            if (!(S.nleaf(cur)[i] & 2)) {
                const int pos = T + (int)S.pk[i];
                S.ns(nxt)[pos] = S.ns(cur)[i]; S.ne(nxt)[pos] = S.ne(cur)[i]; S.nd(nxt)[pos] = S.nd(cur)[i]; S.nleaf(nxt)[pos] = S.nleaf(cur)[i];
            }
        wg_barrier();
        cur = nxt; m = m_new;
        if (N <= m || m == prev) break;
    }

    if (failed) {
        if (tid == 0) { atomicOr(status, 2); *out_cnt = 0; }
        return;
    }
    // ---- 4. best candidate per node: max score, then smallest candidate index
    QT_PROF_TICK(6);
    const int m_out = min(m, L.sel_cap);
    if (m > L.sel_cap && tid == 0) atomicOr(status, 2);
    if (small) {   // the same walk over the LDS copies (a loop of its own: one loop over a pointer chosen at run time would be FLAT accesses)
        for (int i = tid; i < m_out; i += 256) {
            const int s = S.ns(cur)[i], e = S.ne(cur)[i];
            if (s >= n || e > n || s >= e) { atomicOr(status, 8); out_sel[i] = 0; continue; }   // cannot happen: node ranges partition [0, n)
            uint32_t best_id = sid[s], best_pk = spk[s];
            for (int t = s + 1; t < e; ++t) {
                const uint32_t id = sid[t], pk = spk[t];
                const uint32_t sa = pk >> 24, sb = best_pk >> 24;
                if (sa > sb || (sa == sb && id < best_id)) { best_id = id; best_pk = pk; }
            }
            out_sel[i] = (int32_t)best_pk;
        }
    } else {
        for (int i = tid; i < m_out; i += 256) {
            const int s = S.ns(cur)[i], e = S.ne(cur)[i];
            if (s >= n || e > n || s >= e) { atomicOr(status, 8); out_sel[i] = 0; continue; }   // cannot happen: node ranges partition [0, n)
            uint32_t best_id = sidx[s];
            if (best_id >= (uint32_t)n) { atomicOr(status, 8); best_id = (uint32_t)(n - 1); }   // cannot happen: the sort permutes [0, n)
            uint32_t best_pk = cand[best_id];
            for (int t = s + 1; t < e; ++t) {
                uint32_t id = sidx[t];
                if (id >= (uint32_t)n) { atomicOr(status, 8); id = (uint32_t)(n - 1); }
                const uint32_t pk = cand[id];
                const uint32_t sa = pk >> 24, sb = best_pk >> 24;
                if (sa > sb || (sa == sb && id < best_id)) { best_id = id; best_pk = pk; }
            }
            out_sel[i] = (int32_t)best_pk;
        }
    }
    if (tid == 0) *out_cnt = m_out;
    QT_PROF_TICK(7);
    QT_PROF_REPORT();
}

size_t quadtree_scratch_bytes_per_frame(const LevelDev* h_lv, int n_levels) {
    size_t end = 0;
    for (int l = 0; l < n_levels; ++l) end = h_lv[l].qt_off + (size_t)h_lv[l].qt_cap * 20;
    return (end + 255) / 256 * 256;
}

// node arrays for 3 * quota + 8 entries (the bound of the lists, see QtShared), rounded to 8: at K = 1000 (quota 217) 25.5 KB, so that THREE
// workgroups fit the 77 KB two region-growing workgroups leave on a CU (rounded to a power of two it was 34.9 KB: two)
static void qt_layout(int max_quota, int& mn, int& blk) {
    const int want = std::max(256, (3 * max_quota + 8 + 7) / 8 * 8);
    const bool small_blk = want > kQtMaxNodes;                    // a quota above 1960 (plp_orb_create has checked that it fits with the smaller block and that no level has more cells than it holds)
    mn = std::min(small_blk ? kQtMaxNodesLdsSmallBlock : kQtMaxNodes, want); blk = small_blk ? kQtBlkWordsSmall : kQtBlkWords;
}
size_t quadtree_lds_bytes(int max_quota) {
    int mn, blk;
    qt_layout(max_quota, mn, blk);
    return qt_lds_bytes(mn, blk);
}
// More than 64 KB of dynamic LDS (a per-level quota of 730 or more) needs the function's limit raised on the device that launches it: every ORB context does so for
// its own device when it is created and refuses such a quota where that failed (orb_context.hip).
hipError_t quadtree_configure() {
    return hipFuncSetAttribute(reinterpret_cast<const void*>(k_quadtree), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
}

void launch_quadtree(hipStream_t st, const LevelDev* d_lv, int n_levels, int n_cells_total, const uint32_t* cell_cand,
                     const int32_t* cell_count, int32_t* sel, int32_t* sel_count, int total_sel_cap, uint32_t* qt_scratch,
                     size_t qt_scratch_frame_stride, int32_t* status, int B, int max_quota) {
    int mn, blk;
    qt_layout(max_quota, mn, blk);
    hipLaunchKernelGGL(k_quadtree, dim3(n_levels, B), dim3(256), qt_lds_bytes(mn, blk), st, d_lv, n_cells_total, cell_cand, cell_count, sel,
                       sel_count, total_sel_cap, reinterpret_cast<uint8_t*>(qt_scratch), qt_scratch_frame_stride, status, mn, blk);
}

}  // namespace plp
