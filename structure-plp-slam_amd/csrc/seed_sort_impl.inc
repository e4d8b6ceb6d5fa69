// Body of the exact seed sort (seed_sort_kernels.hip includes it once per configuration: SS_NS = namespace, SS_WAVES = waves per workgroup,
// SS_T = entries of the LDS window).
namespace SS_NS {


using seedsort::KeyDesc;
using seedsort::median3_pos;
using seedsort::select64;
using seedsort::select64_top;

constexpr int kSsWaves = SS_WAVES, kSsThreads = 64 * kSsWaves;
typedef uint16_t lrpos_t;
constexpr int kSsT = SS_T;       // LDS window, entries.  A partition in LDS costs about as much per entry as one in global memory (both run on
                                     // barriers and instruction issue, not on bytes), so the window is small: 51 KB of LDS per workgroup leave room for a
                                     // second workgroup -- or the region growers of another batch -- on the CU (24576 entries = 144 KB: 5.05 ms alone but
                                     // +7.4 ms on the step, profiles/r04_seed_sort.md)

constexpr int kSsTask = kSsT < SS_TASK ? kSsT : SS_TASK;   // longest segment one wave partitions (at most 64 chunks = 64 lanes: 4096); longer ones inside the window take the whole workgroup
constexpr int kSsSmall = 64;         // (longest segment one lane sorted until round 6; still the bound of lane_introsort, which only the debug builds call)
constexpr int kSsSub = 256;          // longest segment whose WHOLE SUBTREE one wave finishes by itself (wave_sub_sort): chunk masks and prefix sums in scalar registers,
constexpr int kSubK = kSsSub / 64;   // no queue traffic, no lane-sequential scans.  Round 6: two thirds of a frame's wave tasks and all of its lane segments are of this kind
constexpr int kSsShift = seedsort::kKeyShift;
static_assert(kSsShift == kLsdSeedPixBits, "entry layout = the seed packing of k_lsd_order");
constexpr uint32_t kSsDefBit = 1u << 19;
static_assert(kLsdMaxScaledPixels <= (size_t)kSsDefBit, "pixel index below the defined bit");
// Capacities follow the window (round 6; they were 512 / 1536 for every configuration: 10 KB of the 4-wave kernel's 35 KB of LDS, i.e. of what decides how many
// workgroups share a CU): a wave task has more than kSsSub entries, a listed subtree more than 16, and both lie inside the window.
constexpr int kSsQueue = kSsT <= 4096 ? 128 : 512, kSsSmallCap = kSsT <= 4096 ? 256 : 1536, kSsGStack = 64, kSsWStack = 8;
static_assert((kSsQueue & (kSsQueue - 1)) == 0 && kSsT / (kSsSub + 1) < kSsQueue && kSsT / 17 < kSsSmallCap && kSsT / (kSsTask + 1) < kSsWStack, "queue capacities");
constexpr int kSsChunksW = kSsT / 64 + 1;                                  // chunk slots of an LDS partition
constexpr int kSsMaxChunksG = (int)((kLsdMaxScaledPixels + 63) / 64) + 1;  // of a global one (prefix arrays alias the window)

struct SsCtl {                       // LDS control block
    int bc[8];                       // broadcasts: m, cut, block-scan totals
    int wsum[2][kSsWaves];
    int g_n; int g_first[kSsGStack], g_last[kSsGStack], g_depth[kSsGStack];
    int w_n; int w_first[kSsWStack], w_last[kSsWStack], w_depth[kSsWStack];
    int q_head, q_tail, q_pending, q_open, n_small, small_head, overflow;
    int n_live;                      // entries [n_live, n) are DEAD: right parts of global partitions whose pivot bin lies below the skip key (see wg_partition)
    long long t[24];                      // diagnostics (debug entry only): cycles in {G partitions, window load, workgroup levels, wave tasks, lanes, store}, windows, G partitions; [16..19] of the G partitions: classify, scan, crossing, exchange
};

// dynamic LDS layout (bytes): control block and queues first, the window LAST -- the prefix arrays of a partition in global memory (12 bytes per
// chunk of 64 entries of the segment) take the place of the partner list and the window, which are idle then; for a frame whose seed array has more
// chunks than fit there the host asks for a larger allocation (seed_sort_lds_bytes)
constexpr size_t kOffCtl = 0;
constexpr size_t kOffQ = (sizeof(SsCtl) + 7) / 8 * 8;
constexpr size_t kOffSmall = kOffQ + (size_t)kSsQueue * 8;
constexpr size_t kOffML = (kOffSmall + (size_t)kSsSmallCap * 4 + 7) / 8 * 8;
constexpr size_t kOffMR = kOffML + (size_t)kSsChunksW * 8;
constexpr size_t kOffPA = kOffMR + (size_t)kSsChunksW * 8;
constexpr size_t kOffPBx = kOffPA + (size_t)kSsChunksW * 4;
constexpr size_t kOffPBi = kOffPBx + (size_t)kSsChunksW * 4;
constexpr size_t kOffRpos = (kOffPBi + (size_t)kSsChunksW * 4 + 15) / 16 * 16;
constexpr size_t kOffWin = kOffRpos + ((size_t)(kSsT / 2 + 64) * sizeof(lrpos_t) + 15) / 16 * 16;
constexpr size_t kSsLdsBytes = kOffWin + (size_t)kSsT * 4 + 16;   // + a pad: lane_introsort reads two entries per LDS access, the second may lie one word behind the window
static_assert(kOffRpos + (size_t)kSsMaxChunksG * 12 <= 160 * 1024 && kSsLdsBytes <= 160 * 1024, "LDS of the seed sort");

// A partition in global memory lays out the area from kOffRpos on as: pA, pBx (4 bytes per chunk slot each), the chunk masks when they are held in LDS (16 bytes per
// chunk), pBi.  After the crossing pBi is dead, and what lies from its offset on is the EXCHANGE TILE: two arrays of `ranks` entries, through which the stoppers of
// `ranks` consecutive ranks change sides (wg_partition, "B / C").  Host and device compute the tile from the same two functions.
constexpr int kSsTileMin = 512;      // masks in LDS only where they leave a tile of this many ranks (two barriers and one memory latency per tile; every partition of a 640 x 480 frame but the first)
__host__ __device__ constexpr size_t ss_tile_off(int nch, bool lm) { return (size_t)((nch + 2) & ~1) * 8 + (lm ? (size_t)nch * 16 : 0); }
// a segment of n_seg entries when the area has `area` bytes: *lm = masks in LDS; returns the ranks per tile
__host__ __device__ inline int ss_tile_plan(int n_seg, size_t area, bool* lm) {
    const int nch = (n_seg - 1 + 63) >> 6;
    const size_t offL = ss_tile_off(nch, true), offN = ss_tile_off(nch, false);
    const size_t rL = area > offL ? (area - offL) / 8 : 0, rN = area > offN ? (area - offN) / 8 : 0;
    *lm = rL >= (size_t)kSsTileMin && offL + (size_t)((nch + 2) & ~1) * 4 <= area;   // (... and pBi fits where the tile will be: it has a slot per chunk, a long segment of a large frame more than a short tile)
    return (int)(*lm ? rL : rN);
}
// Without the masks a tile is never short: the area is the larger of what the window phase needs (A) and 12 bytes per chunk slot of the FRAME (lds_bytes), a segment
// has at most the frame's chunks + 1 slots at 8 bytes, so the tile has at least min(A / 24, A / 12 / 2) - 2 ranks
static_assert((kSsLdsBytes - kOffRpos - 16) / 24 >= 64 + 2, "every global partition has an exchange tile");

struct SsMem {
    uint32_t* a;                      // the entries the partition works on (global: the frame's array; LDS: the window)
    void* rpos;                       // LDS partitions: partner positions by rank, uint16_t[] (global partitions exchange entries through an LDS tile: no list)
    unsigned long long *mL, *mR;      // chunk masks of left / right stoppers
    uint32_t *pA, *pBx, *pBi;         // per chunk: left stoppers before it / right stoppers after it / in it and after it (LDS in both cases)
    size_t lds_bytes_g;               // global partitions: bytes of LDS from pA on (prefix arrays, then the masks if they fit)
};

// inclusive scan over the 64 lanes: rows of 16 by DPP row shifts (a lane whose source falls outside its row keeps the 0 passed as `old`), the
// three row totals through v_readlane -- no LDS round trips (six ds_bpermute steps had been a tenth of a small partition)
__device__ __forceinline__ int wave_incl_scan(int v, int lane) {
    v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, false);   // row_shr:1
    v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, false);   // row_shr:2
    v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, false);   // row_shr:4
    v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, false);   // row_shr:8
    const int t0 = __builtin_amdgcn_readlane(v, 15), t1 = __builtin_amdgcn_readlane(v, 31), t2 = __builtin_amdgcn_readlane(v, 47);
    return v + (lane >= 16 ? t0 : 0) + (lane >= 32 ? t1 : 0) + (lane >= 48 ? t2 : 0);
}
__device__ __forceinline__ int wave_max(int v) {   // the same value in every lane
    v = max(v, __builtin_amdgcn_update_dpp(v, v, 0x128, 0xf, 0xf, false));   // row_ror:8
    v = max(v, __builtin_amdgcn_update_dpp(v, v, 0x124, 0xf, 0xf, false));
    v = max(v, __builtin_amdgcn_update_dpp(v, v, 0x122, 0xf, 0xf, false));
    v = max(v, __builtin_amdgcn_update_dpp(v, v, 0x121, 0xf, 0xf, false));
    return max(max(__builtin_amdgcn_readlane(v, 0), __builtin_amdgcn_readlane(v, 16)), max(__builtin_amdgcn_readlane(v, 32), __builtin_amdgcn_readlane(v, 48)));
}
__device__ __forceinline__ unsigned long long readlane64(unsigned long long v, int src) {
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, src), hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), src);
    return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ unsigned long long lanes_below(int lane) { return (1ull << lane) - 1ull; }
// A value every lane of the wave holds (a wave index, a word all lanes read from one LDS address): said so, so that what depends on it -- loop counters,
// bounds, base addresses -- is scalar code instead of 64 identical lanes behind execution masks (round 5: the same one-liner took k_lsd_grow from 155 to 113 VGPRs).
__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ unsigned long long bits_above(unsigned long long m, int lane) { return (m >> lane) >> 1; }
// set bits of a mask below this lane / above it: v_mbcnt (two instructions for a mask in scalar registers) instead of a 64-bit and + two popcounts
__device__ __forceinline__ int below_cnt(unsigned long long m) { return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u)); }
__device__ __forceinline__ int above_cnt(unsigned long long m, int lane) { return __popcll(m) - below_cnt(m) - (int)((m >> lane) & 1ull); }

// Barriers.  wg_barrier() (plp_barrier.hpp) = a HARD `s_waitcnt lgkmcnt(0)` + `__syncthreads()`: the soft wait of __syncthreads()'s own fence was deleted by the compiler
// at the barrier that heads the loop over a frame's global partitions in some builds of this file -- the cause of the fault of rounds 4 - 6 (an experiment build with two
// waves per workgroup in round 4, every build with vector-address accesses to the masks' HBM copy in round 6, the debug entry's kernel always; profiles/r06_seed_sort.md
// section 4).  Between the passes of a partition in GLOBAL memory chunk masks and the entries themselves go from wave to wave through HBM / L2: that
// barrier drains the wave's own stores as well (the memory model lets a workgroup-scope release skip vmcnt because the waves of a workgroup share a CU and its vector L1).
// What stays from the hunt is the CHECK of every partition's swap count and cut (ADVICE r05): damaged masks are never used as addresses, the frame reports status bit 32.
#define SS_PLAIN_BARRIER() wg_barrier()
template <bool G> __device__ __forceinline__ void ss_barrier() {
    if constexpr (G) wg_barrier_after_global_stores(); else wg_barrier();
}

// number of chunks c in [0, nch) with pred(c), for a predicate that is true on a prefix of the chunks: 64 probes per round (one wave)
template <class Pred> __device__ __forceinline__ int wave_count_prefix(int nch, int lane, Pred pred) {
    int lo = 0, hi = nch;              // the count lies in [lo, hi]
    while (lo < hi) {
        const int step = (hi - lo + 63) >> 6, c = lo + lane * step;
        const int t = __popcll(__ballot(c < hi && pred(c)));
        if (t == 0) { hi = lo; break; }
        const int nlo = lo + (t - 1) * step + 1;
        hi = min(hi, lo + t * step);
        lo = nlo;
    }
    return lo;
}

// Whole-workgroup partition of [first, last) (more than 64 entries) around the median of three; returns the cut.  Ends with a barrier.
// Every pass takes U chunks per wave and trip, so that U independent loads (and, in the swap pass, U chains of three dependent ones) are
// in flight per wave: with one chunk per trip the global-memory form ran at one memory latency per 64 entries and wave.
// Global partitions: the entries of the stoppers change sides through an LDS tile of `tile_ranks` ranks per side (ss_tile_plan).
template <bool G, bool LM = false> __device__ __forceinline__ int wg_partition(const SsMem& M, SsCtl* ctl, int first, int last, uint32_t skip_key, bool prof = false, int tile_ranks = 0) {
    long long tp0 = prof ? clock64() : 0;
    auto plap = [&](int k) { if (prof && threadIdx.x == 0) { const long long t1 = clock64(); ctl->t[(G ? 16 : 10) + k] += t1 - tp0; tp0 = t1; } };
    using rpos_t = lrpos_t;
    [[maybe_unused]] constexpr int U = 4;  // chunks per wave and trip: the swap passes ...
    constexpr int UA = G ? 16 : 4;         // ... and the classifying pass (one load per chunk)
    [[maybe_unused]] rpos_t* rpos = G ? nullptr : (rpos_t*)M.rpos + (first >> 1);
    uint32_t* a = M.a;
    const int tid = threadIdx.x, lane = tid & 63, wv = uni(tid >> 6);
    first = uni(first); last = uni(last);
    const int p0 = first + 1, np = last - p0, nch = (np + 63) >> 6, mid = first + (last - first) / 2;
    // Where the chunk masks and prefix arrays of THIS partition live.  In LDS both; a global partition (round 6) packs its prefix arrays at the start of the area
    // the idle window leaves and puts the masks behind them where they leave room for an exchange tile (ss_tile_plan) -- every partition but the first of a 640 x 480 frame:
    // 12 + 16 bytes per chunk of the segment, 41 k entries need 18 KB -- so that the passes below read them from LDS instead of making a round trip through HBM before their entry loads.
    SsMem Q = M;
    if constexpr (G) {
        // pBi comes LAST: only the crossing reads it, so the exchange tile starts where it lies (ss_tile_off)
        const int nchp = (nch + 2) & ~1;
        Q.pA = M.pA; Q.pBx = M.pA + nchp;
        if constexpr (LM) { Q.mL = (unsigned long long*)(M.pA + 2 * nchp); Q.mR = Q.mL + nch; }   // (the caller's choice: ss_tile_plan)
        Q.pBi = (uint32_t*)((unsigned char*)M.pA + ss_tile_off(nch, LM));
    }
    const uint32_t e0 = a[first], ea = a[p0], eb = a[mid], ec = a[last - 1];
    const int m3 = median3_pos(ea >> kSsShift, eb >> kSsShift, ec >> kSsShift, p0, mid, last - 1);
    const uint32_t em = m3 == p0 ? ea : (m3 == mid ? eb : ec), pk = em >> kSsShift;
    // A: stoppers of the array as it is after the median's swap with a[first] (a[m3] = e0; done physically in S)
    for (int c0 = wv * UA; c0 < nch; c0 += kSsWaves * UA) {
        uint32_t e[UA];
#pragma unroll
        for (int u = 0; u < UA; ++u) {
            const int pos = p0 + ((c0 + u) << 6) + lane;
            e[u] = pos < last ? a[pos] : 0u;
        }
#pragma unroll
        for (int u = 0; u < UA; ++u) {
            const int c = c0 + u, pos = p0 + (c << 6) + lane;
            if (c >= nch) break;
            const bool valid = pos < last;
            const uint32_t k = (pos == m3 ? e0 : e[u]) >> kSsShift;
            const unsigned long long mL = __ballot(valid && k <= pk), mR = __ballot(valid && k >= pk);
            if (lane == 0) { Q.mL[c] = mL; Q.mR[c] = mR; Q.pA[c] = (uint32_t)__popcll(mL); Q.pBx[c] = (uint32_t)__popcll(mR); }   // (the counts: what the scan below starts from)
        }
    }
    ss_barrier<G>();
    plap(0);
    // S: per chunk the left stoppers before it and the right stoppers after it.  A thread owns `cpt` consecutive chunks; their popcounts wait in the
    // prefix arrays themselves (LDS) while the block scans the threads' totals, and are replaced by the prefix values afterwards (a thread re-reads only
    // what it wrote: no barrier for that).  Until round 5 they waited in per-thread register arrays sized for the LARGEST frame (kSsCpt = 32 entries x 2 with
    // four waves, 64 x 2 with two): the kernel's register peak -- and the one code shape every build that faulted had in common (DESIGN.md section 5).
    {
        const int cpt = (nch + kSsThreads - 1) / kSsThreads, c0 = tid * cpt;
        int cl = 0, cr = 0;
        // the popcounts of a thread's chunks: pass A left them in the prefix arrays (round 6; until then this pass re-read the masks -- from HBM in a global partition)
        for (int q = 0; q < cpt; ++q) { const int c = c0 + q; if (c < nch) { cl += (int)Q.pA[c]; cr += (int)Q.pBx[c]; } }
        const int il = wave_incl_scan(cl, lane), ir = wave_incl_scan(cr, lane);
        if (lane == 63) { ctl->wsum[0][wv] = il; ctl->wsum[1][wv] = ir; }
        SS_PLAIN_BARRIER();
        int bl = 0, br = 0, totR = 0;
        for (int w = 0; w < kSsWaves; ++w) { const int sl = ctl->wsum[0][w], sr = ctl->wsum[1][w]; if (w < wv) { bl += sl; br += sr; } totR += sr; }
        int runL = bl + il - cl, runR = br + ir - cr;
        for (int q = 0; q < cpt; ++q) {
            const int c = c0 + q;
            if (c < nch) {
                const int kl = (int)Q.pA[c], kr = (int)Q.pBx[c];
                Q.pA[c] = (uint32_t)runL;
                runL += kl; runR += kr;
                Q.pBx[c] = (uint32_t)(totR - runR);
                Q.pBi[c] = (uint32_t)(totR - runR + kr);      // right stoppers in this chunk and after it
            }
        }
        if (tid == kSsThreads - 1) { ctl->bc[2] = runL; ctl->bc[4] = totR; }   // all left stoppers, all right stoppers
    }
    SS_PLAIN_BARRIER();
    plap(1);
    if (wv == 0) {   // the crossing: m, the cut, the median's swap
        const int totL = uni(ctl->bc[2]);
        const int cs = wave_count_prefix(nch, lane, [&](int c) { return Q.pA[c] <= Q.pBi[c]; }) - 1;
        const unsigned long long sL = Q.mL[cs], sR = Q.mR[cs];
        const int sA = (int)Q.pA[cs], sB = (int)Q.pBi[cs];
        int v = min(sA + below_cnt(sL), sB - below_cnt(sR));
        const int m = max(wave_max(v), min(sA + __popcll(sL), sB - __popcll(sR)));
        int cut;
        if (m == 0) {
            const int c = wave_count_prefix(nch, lane, [&](int c) { return (c + 1 < nch ? (int)Q.pA[c + 1] : totL) == 0; });   // chunks before the first left stopper
            cut = p0 + (c << 6) + __builtin_ctzll(Q.mL[c]);
        } else {
            int Lm = 0x7fffffff;
            if (m < totL) {
                const int c = wave_count_prefix(nch, lane, [&](int c) { return (int)Q.pA[c] <= m; }) - 1;
                Lm = p0 + (c << 6) + select64(Q.mL[c], m - (int)Q.pA[c]);
            }
            const int c = wave_count_prefix(nch, lane, [&](int c) { return (int)Q.pBx[c] > m - 1; });
            cut = min(Lm, p0 + (c << 6) + select64_top(Q.mR[c], m - 1 - (int)Q.pBx[c]));
        }
        // (ADVICE r05) what the swap passes and the caller are about to trust is checked once per partition, on scalars: at most min(totL, totR) swaps, a cut inside
        // (first, last].  A violation means the masks / prefix arrays are damaged (the fault of the 2-wave experiment build, DESIGN.md section 5): the partition swaps
        // nothing, the frame stops sorting (every loop above reads ctl->overflow at its next barrier) and reports status bit 32.
        const int totR = uni(ctl->bc[4]);
        const bool sane = m >= 0 && m <= min(totL, totR) && cut > first && cut <= last;
        if (lane == 0) {
            if (sane) { a[first] = em; a[m3] = e0; ctl->bc[0] = m; ctl->bc[1] = cut; }
            else { ctl->bc[0] = 0; ctl->bc[1] = last; if (!ctl->overflow) { ctl->overflow = 1; ctl->bc[6] = m; ctl->bc[7] = cut; } }
            ctl->bc[3] = (int)pk;
            if constexpr (G) {
                // A pivot bin below the skip key: the right part (keys <= pivot) holds undefined pixels only and is never looked at again -- not by a partition (the
                // caller does not push it) and, once it is the END of the live array, not by the counting sort either (k_lsd_order_entries reads [0, n_live)).
                // Then nothing has to be stored there: the right stoppers still hand their entries to the left part, the left stoppers' entries (undefined pixels)
                // are dropped.  Everything to the right of a segment whose pivot is below the skip key is dead already (its keys are at most this segment's smallest:
                // some ancestor's pivot was below the key too), so `last == n_live` holds whenever the pivot is -- checked, not assumed.
                const bool dead = sane && pk < skip_key && last == ctl->n_live;
                ctl->bc[5] = dead ? 1 : 0;
                if (dead) ctl->n_live = cut;
            }
        }
    }
    ss_barrier<G>();
    plap(2);
    const int m = uni(ctl->bc[0]), cut = uni(ctl->bc[1]);
    if constexpr (G) {
        // Global memory, exchange through LDS.  Until round 6 the swap pass was a chain of dependent scattered accesses per stopper (partner position from a rank-indexed
        // list, the partner's entry, two scattered stores); round 6 handed the entries over BY RANK through two lists in HBM -- coalesced, no address from memory, but a
        // load and a store to export an entry and a load and a store to import it, in two latency-bound passes.  The lists only took a value from one wave of the
        // workgroup to another: LDS does that.  The ranks [0, m) are cut into tiles of R; the stoppers of a tile load their own
        // entries and put them into tileL / tileR by rank, and after a barrier take the other side's entry of their rank from there and store it to their own position:
        // one load and one store per moved entry.  Ranks rise with the position on the left side and towards the left on the right side, so the stoppers of a tile lie in
        // one run of chunks per side; [cL, cLe) and (cRe, cR] are found from the prefix arrays by a cursor that only moves forward (a chunk that straddles a tile's border
        // is the last chunk of one tile and the first of the next; a lane acts in the tile its rank falls in).  The loads take the whole chunk, so that they do not wait
        // for the chunk's mask (in HBM in a frame's first partition): a chunk of a tile is half stoppers, the lines are the same.
        constexpr int UT = 4;
        const int R = uni(tile_ranks);
        uint32_t* tileL = Q.pBi; uint32_t* tileR = tileL + R;
        const bool dead = uni(ctl->bc[5]) != 0;
        const int wr = kSsWaves - 1 - wv;                            // the right side's chunks go to the waves in reverse order: a tile of a few chunks per side keeps all waves busy
        int cL = 0, cR = nch - 1;                                    // pA[cL] <= r0 and pBx[cR] <= r0: the chunks that hold rank r0
        for (int r0 = 0; r0 < m; r0 += R) {
            const int r1 = min(r0 + R, m);
            int cLe = cL, cRe = cR;
            while (true) { const int c = cLe + lane, k = __popcll(__ballot(c < nch && (int)Q.pA[c] < r1)); cLe += k; if (k < 64) break; }
            while (true) { const int c = cRe - lane, k = __popcll(__ballot(c >= 0 && (int)Q.pBx[c] < r1)); cRe -= k; if (k < 64) break; }
            cLe = uni(cLe); cRe = uni(cRe);
            // one side's chunks of the tile, counted from the cursor (chunk cb + j on the left, cb - j on the right); PUT: entry -> tile, else: the other side's entry -> position
            auto pass = [&](auto is_left, auto is_put) {
                constexpr bool LEFT = decltype(is_left)::value, PUT = decltype(is_put)::value;
                uint32_t* mine = LEFT ? tileL : tileR; const uint32_t* theirs = LEFT ? tileR : tileL;
                const unsigned long long* msk = LEFT ? Q.mL : Q.mR; const uint32_t* pre = LEFT ? Q.pA : Q.pBx;
                const int cb = LEFT ? cL : cR, nj = LEFT ? cLe - cL : cR - cRe;
                for (int j0 = (LEFT ? wv : wr) * UT; j0 < nj; j0 += kSsWaves * UT) {
                    [[maybe_unused]] uint32_t e[UT];
                    if constexpr (PUT) {
#pragma unroll
                        for (int u = 0; u < UT; ++u) {
                            const int pos = p0 + ((LEFT ? cb + j0 + u : cb - j0 - u) << 6) + lane;
                            e[u] = (j0 + u < nj && pos < last) ? a[pos] : 0u;
                        }
                    }
#pragma unroll
                    for (int u = 0; u < UT; ++u) {
                        if (j0 + u >= nj) break;
                        const int c = LEFT ? cb + j0 + u : cb - j0 - u;
                        const unsigned long long mk = msk[c];
                        const int r = (int)pre[c] + (LEFT ? below_cnt(mk) : above_cnt(mk, lane));
                        if (((mk >> lane) & 1ull) && r >= r0 && r < r1) {
                            if constexpr (PUT) mine[r - r0] = e[u];
                            else a[p0 + (c << 6) + lane] = theirs[r - r0];
                        }
                    }
                }
            };
            // B: every stopper of the tile puts its entry into the tile (the left stoppers of a partition whose right part is dead need not: their entries are dropped)
            if (!dead) pass(std::true_type{}, std::true_type{});
            pass(std::false_type{}, std::true_type{});
            wg_barrier();
            // C: ... and takes the other side's entry of its rank into its own position (nothing is stored into a dead right part)
            pass(std::true_type{}, std::false_type{});
            if (!dead) pass(std::false_type{}, std::false_type{});
            wg_barrier();                                            // (the tile is written again)
            cL = cLe - 1; cR = cRe + 1;
        }
        ss_barrier<G>();
        plap(3);
    } else {
    // B: the right stoppers of rank < m leave their positions in the rank-indexed list (chunks from the right end; those further left only hold higher ranks)
    for (int c0 = nch - 1 - wv * U; c0 >= 0; c0 -= kSsWaves * U) {
        if (uni((int)Q.pBx[c0]) >= m) break;
        unsigned long long mR[U]; int bx[U];
#pragma unroll
        for (int u = 0; u < U; ++u) { const int c = c0 - u; mR[u] = c >= 0 ? Q.mR[c] : 0ull; bx[u] = c >= 0 ? (int)Q.pBx[c] : m; }
#pragma unroll
        for (int u = 0; u < U; ++u)
            if ((mR[u] >> lane) & 1ull) {
                const int rank = bx[u] + above_cnt(mR[u], lane);
                if (rank < m) rpos[rank] = (rpos_t)(p0 + ((c0 - u) << 6) + lane);
            }
    }
    ss_barrier<G>();
    plap(3);
    // C: the left stoppers of rank < m swap with their partners
    for (int c0 = wv * U; c0 < nch; c0 += kSsWaves * U) {
        if (uni((int)Q.pA[c0]) >= m) break;
        int i[U], j[U]; uint32_t vi[U], vj[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int c = c0 + u;
            i[u] = -1;
            if (c < nch) {
                const unsigned long long mL = Q.mL[c];
                const int rank = (int)Q.pA[c] + below_cnt(mL);
                if (((mL >> lane) & 1ull) && rank < m) i[u] = rank;
            }
        }
        // a stopper's own entry does not depend on its partner's position: both loads of a lane go out together, the partner's entry follows
#pragma unroll
        for (int u = 0; u < U; ++u) if (i[u] >= 0) { j[u] = (int)rpos[i[u]]; vi[u] = a[p0 + ((c0 + u) << 6) + lane]; }
#pragma unroll
        for (int u = 0; u < U; ++u) if (i[u] >= 0) vj[u] = a[j[u]];
#pragma unroll
        for (int u = 0; u < U; ++u) if (i[u] >= 0) { a[p0 + ((c0 + u) << 6) + lane] = vj[u]; a[j[u]] = vi[u]; }
    }
    ss_barrier<G>();
    plap(4);
    }
    if (prof && threadIdx.x == 0) ctl->t[(G ? 16 : 10) + 5] += 1;
    return cut;
}

// One wave partitions [first, last) of the LDS window, 65 .. kSsTask entries: chunk c's masks and prefix sums live in lane c.
// Returns the cut, or -1 when the segment held equal keys and was FINISHED here (seed_sort_model.hpp uniform_final_pos): `depth` partitions are
// left in the recursion budget, the shortcut is taken only where the library would not have run out of it either.
__device__ __forceinline__ int wave_partition(uint32_t* a, lrpos_t* rpos_all, int first, int last, int depth, int lane, uint32_t skip_key, uint32_t* pivot_key) {
    lrpos_t* rpos = rpos_all + (first >> 1);
    const int p0 = first + 1, np = last - p0, nch = (np + 63) >> 6, mid = first + (last - first) / 2;
    const uint32_t e0 = a[first], ea = a[p0], eb = a[mid], ec = a[last - 1];
    const int m3 = median3_pos(ea >> kSsShift, eb >> kSsShift, ec >> kSsShift, p0, mid, last - 1);
    const uint32_t em = m3 == p0 ? ea : (m3 == mid ? eb : ec), pk = em >> kSsShift;
    *pivot_key = pk;
    unsigned long long myL = 0, myR = 0;
    constexpr int U = 4;                                         // chunks per trip: their loads are in flight together
    for (int c0 = 0; c0 < nch; c0 += U) {
        uint32_t e[U];
#pragma unroll
        for (int u = 0; u < U; ++u) { const int pos = p0 + ((c0 + u) << 6) + lane; e[u] = pos < last ? a[pos] : 0u; }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int c = c0 + u, pos = p0 + (c << 6) + lane;
            if (c >= nch) break;
            const bool valid = pos < last;
            const uint32_t k = (pos == m3 ? e0 : e[u]) >> kSsShift;
            const unsigned long long mL = __ballot(valid && k <= pk), mR = __ballot(valid && k >= pk);
            if (lane == c) { myL = mL; myR = mR; }
        }
    }
    const int cl = __popcll(myL), cr = __popcll(myR);
    const int il = wave_incl_scan(cl, lane), ir = wave_incl_scan(cr, lane);
    const int totL = __builtin_amdgcn_readlane(il, 63), totR = __builtin_amdgcn_readlane(ir, 63);
    if (totL == np && totR == np && last - first <= seedsort::kUniformMax && seedsort::uniform_levels(last - first) <= depth) {
        if (pk < skip_key) return -1;                            // equal keys below the skip key: no defined pixel here
        constexpr int K = seedsort::kUniformMax / 64;
        uint32_t v[K]; int dst[K];
        const int nj = (last - first + 63) >> 6;                 // entries per lane this segment needs (most such segments are short)
#pragma unroll
        for (int j = 0; j < K; ++j) { if (j >= nj) break; const int x = first + (j << 6) + lane; v[j] = x < last ? a[x] : 0u; }
#pragma unroll
        for (int j = 0; j < K; ++j) { if (j >= nj) break; const int x = first + (j << 6) + lane; dst[j] = x < last ? seedsort::uniform_final_pos(x, first, last) : -1; }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // every entry is read before the first one is overwritten
#pragma unroll
        for (int j = 0; j < K; ++j) { if (j >= nj) break; if (dst[j] >= 0) a[dst[j]] = v[j]; }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        return -1;
    }
    const int A = il - cl, Bx = totR - ir;                      // left stoppers before chunk `lane`, right stoppers after it
    const int cs = __builtin_amdgcn_readfirstlane(__popcll(__ballot(lane < nch && A <= Bx + cr)) - 1);
    const unsigned long long sL = readlane64(myL, cs), sR = readlane64(myR, cs);
    const int sA = __builtin_amdgcn_readlane(A, cs), sB = __builtin_amdgcn_readlane(Bx, cs) + __popcll(sR);
    const int v = min(sA + below_cnt(sL), sB - below_cnt(sR));
    const int m = __builtin_amdgcn_readfirstlane(max(wave_max(v), min(sA + __popcll(sL), sB - __popcll(sR))));
    int cut;
    if (m == 0) {
        const int c = __builtin_amdgcn_readfirstlane(__builtin_ctzll(__ballot(lane < nch && cl > 0)));
        cut = p0 + (c << 6) + __builtin_ctzll(readlane64(myL, c));
    } else {
        int Lm = 0x7fffffff;
        if (m < totL) {
            const int c = __builtin_amdgcn_readfirstlane(__popcll(__ballot(lane < nch && A <= m)) - 1);
            Lm = p0 + (c << 6) + select64(readlane64(myL, c), m - __builtin_amdgcn_readlane(A, c));
        }
        const int c = __builtin_amdgcn_readfirstlane(__popcll(__ballot(lane < nch && Bx > m - 1)));
        cut = min(Lm, p0 + (c << 6) + select64_top(readlane64(myR, c), m - 1 - __builtin_amdgcn_readlane(Bx, c)));
    }
    if (lane == 0) { a[first] = em; a[m3] = e0; }
    for (int c = nch - 1; c >= 0; --c) {
        const int bx = __builtin_amdgcn_readlane(Bx, c);
        if (bx >= m) break;
        const unsigned long long mR = readlane64(myR, c);
        if ((mR >> lane) & 1ull) {
            const int rank = bx + above_cnt(mR, lane);
            if (rank < m) rpos[rank] = (lrpos_t)(p0 + (c << 6) + lane);
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    for (int c0 = 0; c0 < nch; c0 += U) {
        if (__builtin_amdgcn_readlane(A, c0) >= m) break;
        int i[U], j[U]; uint32_t vi[U], vj[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int c = min(c0 + u, 63);
            const unsigned long long mL = c0 + u < nch ? readlane64(myL, c) : 0ull;
            const int rank = __builtin_amdgcn_readlane(A, c) + below_cnt(mL);
            i[u] = (((mL >> lane) & 1ull) && rank < m) ? rank : -1;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) if (i[u] >= 0) { j[u] = (int)rpos[i[u]]; i[u] = p0 + ((c0 + u) << 6) + lane; }
#pragma unroll
        for (int u = 0; u < U; ++u) if (i[u] >= 0) { vi[u] = a[i[u]]; vj[u] = a[j[u]]; }
#pragma unroll
        for (int u = 0; u < U; ++u) if (i[u] >= 0) { a[i[u]] = vj[u]; a[j[u]] = vi[u]; }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    return cut;
}

// One lane: std::__introsort_loop on [first, last) of the LDS window, 17 .. kSsSmall entries, `depth` partitions left in the budget.
// The larger part waits, the smaller is continued: at most two parts wait at any time (each has more than 16 of at most 64 entries).
__device__ __forceinline__ void lane_introsort(uint32_t* v, int first, int last, int depth, uint32_t skip_key) {
    const KeyDesc comp;
    int pf0 = 0, pl0 = 0, pd0 = 0, pf1 = 0, pl1 = 0, pd1 = 0, np = 0;
    while (true) {
        while (last - first > 16) {
            if (depth == 0) { libstdcxx::heap_sort(v, first, last, comp); break; }
            --depth;
            const int mid = first + (last - first) / 2, a = first + 1, c = last - 1;
            const int m3 = median3_pos(v[a] >> kSsShift, v[mid] >> kSsShift, v[c] >> kSsShift, a, mid, c);
            { const unsigned t = v[first]; v[first] = v[m3]; v[m3] = t; }
            const unsigned pv = v[first];
            int lo = first + 1, hi = last;
            while (true) {
                // two entries per LDS read in both scans (the chain of dependent reads is what a lane spends its time in): the extra entry may lie one
                // position outside the segment -- inside the workgroup's LDS: the window is followed by a pad word (kSsLdsBytes), and position 0 is
                // never the lower end of the downward scan (hi - 1 >= first + 1) -- and is only looked at if the scan gets there
                while (true) { const unsigned a0 = v[lo], a1 = v[lo + 1]; if (!comp(a0, pv)) break; ++lo; if (!comp(a1, pv)) break; ++lo; }
                --hi;
                while (true) { const unsigned b0 = v[hi], b1 = v[hi - 1]; if (!comp(pv, b0)) break; --hi; if (!comp(pv, b1)) break; --hi; }
                if (!(lo < hi)) break;
                const unsigned t = v[lo]; v[lo] = v[hi]; v[hi] = t;
                ++lo;
            }
            if ((pv >> kSsShift) < skip_key) { last = lo; continue; }   // the right part holds no defined pixel
            int wf, wl;                                          // the part that waits
            if (lo - first >= last - lo) { wf = first; wl = lo; first = lo; } else { wf = lo; wl = last; last = lo; }
            if (wl - wf > 16) {
                if (np == 0) { pf0 = wf; pl0 = wl; pd0 = depth; } else { pf1 = wf; pl1 = wl; pd1 = depth; }
                ++np;
            }
        }
        if (np == 0) break;
        --np;
        if (np == 0) { first = pf0; last = pl0; depth = pd0; } else { first = pf1; last = pl1; depth = pd1; }
    }
}

// position of the k-th set bit of a wave-uniform mask counted from bit 0 / from bit 63, by one ballot (m has more than k bits set): the scalar popcount ladder
// of select64 is ~30 dependent scalar instructions, this is three vector ones and a find-first
__device__ __forceinline__ int select64_b(unsigned long long m, int k, int lane) {
    return __builtin_ctzll(__ballot(((m >> lane) & 1ull) && below_cnt(m) == k));
}
__device__ __forceinline__ int select64_top_b(unsigned long long m, int k, int lane) {
    return __builtin_ctzll(__ballot(((m >> lane) & 1ull) && above_cnt(m, lane) == k));
}

// One wave: std::__introsort_loop on [first, last) of the LDS window, 17 .. 64 entries, IN REGISTERS: lane i holds a[first + i] from the one load to the one store, every
// partition of the subtree works on lane masks (the segment [lo, hi) in lane coordinates), and a partition's swaps are three trips through the LDS crossbar
// (ds_permute / ds_bpermute: no LDS memory, no address arithmetic): the right and left stoppers of rank r push their lane numbers to lane r, a stopper pulls its
// partner's lane from the lane of its rank, then its partner's entry.  ~90 instructions per partition where one lane per segment (rounds 4-5) ran a chain of dependent
// LDS reads per entry in one lane of sixty-four.  Same arithmetic and rules as wave_sub_sort below.
__device__ __forceinline__ void wave_reg_sort(uint32_t* a, int first, int last, int depth, int lane, uint32_t skip_key, SsCtl* ctl, bool prof = false) {
    const long long tr0 = prof ? clock64() : 0;
    int nparts = 0;
    const int base = uni(first), n0 = uni(last - first);
    uint32_t e = lane < n0 ? a[base + lane] : 0u;
    int lo = 0, hi = n0;
    depth = uni(depth);
    uint32_t st0 = 0, st1 = 0, st2 = 0, st3 = 0;                  // waiting parts: lo | (n - 1) << 8 | depth << 16
    int sp = 0;
    while (true) {
        while (hi - lo > 16) {
            if (depth == 0) {                                    // the budget ran out (never on an image): through LDS, one lane runs the library's heap sort
                if (lane < n0) a[base + lane] = e;
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                if (lane == 0) libstdcxx::heap_sort(a, base + lo, base + hi, KeyDesc());
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                e = lane < n0 ? a[base + lane] : 0u;
                break;
            }
            ++nparts;
            const int p0 = lo + 1, np = hi - p0, mid = lo + (hi - lo) / 2;
            const uint32_t e0 = (uint32_t)__builtin_amdgcn_readlane((int)e, lo), ea = (uint32_t)__builtin_amdgcn_readlane((int)e, p0);
            const uint32_t eb = (uint32_t)__builtin_amdgcn_readlane((int)e, mid), ec = (uint32_t)__builtin_amdgcn_readlane((int)e, hi - 1);
            const int m3 = median3_pos(ea >> kSsShift, eb >> kSsShift, ec >> kSsShift, p0, mid, hi - 1);
            const uint32_t em = m3 == p0 ? ea : (m3 == mid ? eb : ec), pk = em >> kSsShift;
            const bool in = lane >= p0 && lane < hi;
            const uint32_t es = lane == lo ? em : (lane == m3 ? e0 : e);       // the array after the median's swap with a[first]
            const uint32_t k = es >> kSsShift;
            const unsigned long long mL = __ballot(in && k <= pk), mR = __ballot(in && k >= pk);
            const int totL = __popcll(mL), totR = __popcll(mR);
            if (totL == np && totR == np && seedsort::uniform_levels(hi - lo) <= depth) {   // equal keys: closed form (on the array BEFORE the median's swap)
                if (pk >= skip_key) {
                    const int dst = (lane >= lo && lane < hi) ? seedsort::uniform_final_pos(lane, lo, hi) : lane;
                    e = (uint32_t)__builtin_amdgcn_ds_permute(dst << 2, (int)e);
                }
                break;
            }
            const int rankL = below_cnt(mL), rankR = above_cnt(mR, lane);
            const int m = uni(wave_max(min(rankL, totR - below_cnt(mR))));    // (the term of position 64 is min(totL, 0))
            int cut;
            if (m == 0) cut = __builtin_ctzll(mL);
            else {
                cut = select64_top_b(mR, m - 1, lane);
                if (m < totL) cut = min(cut, select64_b(mL, m, lane));
            }
            cut = uni(cut);
            const bool isL = ((mL >> lane) & 1ull) && rankL < m, isR = ((mR >> lane) & 1ull) && rankR < m;   // never both: L[r] < cut <= R[r] for r < m
            // lane r < m learns L[r] and R[r] (m <= 32: lane 63 takes what the others push); a stopper pulls its partner's lane from the lane of its rank
            const int Lp = __builtin_amdgcn_ds_permute((isL ? rankL : 63) << 2, lane), Rp = __builtin_amdgcn_ds_permute((isR ? rankR : 63) << 2, lane);
            const int Q = __builtin_amdgcn_ds_bpermute((isL ? rankL : rankR) << 2, Lp | (Rp << 8));
            const int src = isL ? (Q >> 8) & 0xff : (isR ? Q & 0xff : lane);
            e = (uint32_t)__builtin_amdgcn_ds_bpermute(src << 2, (int)es);
            --depth;
            const int nl = cut - lo, nr = pk >= skip_key ? hi - cut : 0;
            const bool goL = nl > 16, goR = nr > 16;
            if (goL && goR) {
                const bool left_waits = nl >= nr;
                const int wf = left_waits ? lo : cut, wn = left_waits ? nl : nr;
                if (sp >= 4) { if (lane == 0) ctl->overflow = 7; sp = 0; hi = lo; break; }   // (cannot happen: 64 entries, a waiting part at least twice the part below it, parts above 16)
                st3 = st2; st2 = st1; st1 = st0; st0 = (uint32_t)wf | ((uint32_t)(wn - 1) << 8) | ((uint32_t)depth << 16); ++sp;
                if (left_waits) lo = cut; else hi = cut;
            } else if (goL) hi = cut;
            else if (goR) lo = cut;
            else break;
        }
        if (sp == 0) break;
        --sp;
        lo = (int)(st0 & 0xffu); hi = lo + (int)((st0 >> 8) & 0xffu) + 1; depth = (int)(st0 >> 16);
        st0 = st1; st1 = st2; st2 = st3;
    }
    if (lane < n0) a[base + lane] = e;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    if (prof && lane == 0) { atomicAdd((unsigned long long*)&ctl->t[10], (unsigned long long)(clock64() - tr0)); atomicAdd((unsigned long long*)&ctl->t[11], 1ull); atomicAdd((unsigned long long*)&ctl->t[12], (unsigned long long)nparts); }
}

// One wave: std::__introsort_loop on [first, last) of the LDS window, 17 .. kSsSub entries, `depth` partitions left in the budget -- the whole subtree, depth first,
// with a stack of at most five waiting parts in scalar registers (the smaller part is continued, so a waiting part is at least twice the one below it).  A partition
// of at most four chunks keeps its chunk masks, popcounts and prefix sums in SCALAR registers (wave_partition spreads them over lanes for up to 64 chunks and pays
// readlanes for every use; one lane per segment, the form of rounds 4-5 for <= 64 entries, is a chain of dependent LDS reads run by one lane in sixty-four).
// Same arithmetic as wave_partition / seed_sort_model.hpp partition_model; same rules for equal keys (closed form) and for parts below the skip key (left alone).
__device__ __forceinline__ void wave_sub_sort(uint32_t* a, lrpos_t* rpos_all, int first, int last, int depth, int lane, uint32_t skip_key, SsCtl* ctl, bool prof = false) {
    const long long ts0 = prof ? clock64() : 0;
    int nparts = 0;
    uint32_t st0 = 0, st1 = 0, st2 = 0, st3 = 0, st4 = 0;       // waiting parts: first | (n - 1) << 16 | depth << 24, st0 = top
    int sp = 0;
    first = uni(first); last = uni(last); depth = uni(depth);
    while (true) {
        while (last - first > 16) {
            if (last - first <= 64) { wave_reg_sort(a, first, last, depth, lane, skip_key, ctl, prof); break; }   // the rest of this branch of the tree: in registers
            if (depth == 0) {
                if (lane == 0) libstdcxx::heap_sort(a, first, last, KeyDesc());
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                break;
            }
            ++nparts;
            const int p0 = first + 1, np = last - p0, mid = first + (last - first) / 2;
            // the pivot candidates and a[first] with ONE LDS access (lanes 0..3), handed round by readlane
            const uint32_t q4 = a[lane == 0 ? first : (lane == 1 ? p0 : (lane == 2 ? mid : last - 1))];
            const uint32_t e0 = (uint32_t)__builtin_amdgcn_readlane((int)q4, 0), ea = (uint32_t)__builtin_amdgcn_readlane((int)q4, 1);
            const uint32_t eb = (uint32_t)__builtin_amdgcn_readlane((int)q4, 2), ec = (uint32_t)__builtin_amdgcn_readlane((int)q4, 3);
            const int m3 = median3_pos(ea >> kSsShift, eb >> kSsShift, ec >> kSsShift, p0, mid, last - 1);
            const uint32_t em = m3 == p0 ? ea : (m3 == mid ? eb : ec), pk = em >> kSsShift;
            uint32_t e[kSubK];
#pragma unroll
            for (int u = 0; u < kSubK; ++u) { const int pos = p0 + (u << 6) + lane; e[u] = pos < last ? a[pos] : 0u; }
            unsigned long long mL[kSubK], mR[kSubK];
            int cl[kSubK], cr[kSubK];
#pragma unroll
            for (int u = 0; u < kSubK; ++u) {
                mL[u] = 0ull; mR[u] = 0ull;
                if ((u << 6) < np) {
                    const int pos = p0 + (u << 6) + lane;
                    if (pos == m3) e[u] = e0;                     // the array as it is after the median's swap with a[first]
                    const uint32_t k = e[u] >> kSsShift;
                    mL[u] = __ballot(pos < last && k <= pk); mR[u] = __ballot(pos < last && k >= pk);
                }
                cl[u] = __popcll(mL[u]); cr[u] = __popcll(mR[u]);
            }
            int A[kSubK], Bx[kSubK];                              // left stoppers before chunk u, right stoppers after it
            A[0] = 0;
#pragma unroll
            for (int u = 1; u < kSubK; ++u) A[u] = A[u - 1] + cl[u - 1];
            Bx[kSubK - 1] = 0;
#pragma unroll
            for (int u = kSubK - 2; u >= 0; --u) Bx[u] = Bx[u + 1] + cr[u + 1];
            const int totL = A[kSubK - 1] + cl[kSubK - 1], totR = Bx[0] + cr[0];
            if (totL == np && totR == np && seedsort::uniform_levels(last - first) <= depth) {   // equal keys: where every entry ends is a function of its position
                if (pk >= skip_key) {
                    uint32_t v[kSubK]; int dst[kSubK];
#pragma unroll
                    for (int j = 0; j < kSubK; ++j) { const int x = first + (j << 6) + lane; v[j] = x < last ? a[x] : 0u; dst[j] = x < last ? seedsort::uniform_final_pos(x, first, last) : -1; }
                    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // every entry is read before the first one is overwritten
#pragma unroll
                    for (int j = 0; j < kSubK; ++j) if (dst[j] >= 0) a[dst[j]] = v[j];
                    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                }
                break;
            }
            // the crossing chunk: the last one with A <= right stoppers in it and after it (true on a prefix of the chunks, at chunk 0 always)
            int cs = 0;
#pragma unroll
            for (int u = 1; u < kSubK; ++u) if ((u << 6) < np && A[u] <= Bx[u] + cr[u]) cs = u;
            unsigned long long sL = mL[0], sR = mR[0]; int sA = 0, sB = Bx[0] + cr[0];
#pragma unroll
            for (int u = 1; u < kSubK; ++u) if (cs == u) { sL = mL[u]; sR = mR[u]; sA = A[u]; sB = Bx[u] + cr[u]; }
            const int vx = min(sA + below_cnt(sL), sB - below_cnt(sR));
            const int m = uni(max(wave_max(vx), min(sA + __popcll(sL), sB - __popcll(sR))));
            int cut;
            if (m == 0) {
                int c = kSubK - 1;
#pragma unroll
                for (int u = kSubK - 2; u >= 0; --u) if (cl[u] > 0) c = u;
                unsigned long long mc = mL[0];
#pragma unroll
                for (int u = 1; u < kSubK; ++u) if (c == u) mc = mL[u];
                cut = p0 + (c << 6) + __builtin_ctzll(mc);
            } else {
                int Lm = 0x7fffffff;
                if (m < totL) {                                  // the chunk that holds the left stopper of rank m: the last one with A <= m
                    int c = 0;
#pragma unroll
                    for (int u = 1; u < kSubK; ++u) if ((u << 6) < np && A[u] <= m) c = u;
                    unsigned long long mc = mL[0]; int ac = 0;
#pragma unroll
                    for (int u = 1; u < kSubK; ++u) if (c == u) { mc = mL[u]; ac = A[u]; }
                    Lm = p0 + (c << 6) + select64_b(mc, m - ac, lane);
                }
                int c = 0;                                       // the right stopper of rank m - 1: the first chunk with at most m - 1 of them after it
#pragma unroll
                for (int u = 0; u < kSubK - 1; ++u) if (Bx[u] > m - 1) c = u + 1;
                unsigned long long mc = mR[0]; int bc = Bx[0];
#pragma unroll
                for (int u = 1; u < kSubK; ++u) if (c == u) { mc = mR[u]; bc = Bx[u]; }
                cut = min(Lm, p0 + (c << 6) + select64_top_b(mc, m - 1 - bc, lane));
            }
            cut = uni(cut);
            if (lane == 0) { a[first] = em; a[m3] = e0; }        // (LDS accesses of a wave are carried out in order: the swaps below come after these two)
            lrpos_t* rpos = rpos_all + (first >> 1);
#pragma unroll
            for (int u = 0; u < kSubK; ++u)
                if ((u << 6) < np && Bx[u] < m && ((mR[u] >> lane) & 1ull)) {
                    const int rank = Bx[u] + above_cnt(mR[u], lane);
                    if (rank < m) rpos[rank] = (lrpos_t)(p0 + (u << 6) + lane);
                }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            int jj[kSubK]; uint32_t vj[kSubK];
#pragma unroll
            for (int u = 0; u < kSubK; ++u) {
                jj[u] = -1;
                if ((u << 6) < np && A[u] < m && ((mL[u] >> lane) & 1ull)) {
                    const int rank = A[u] + below_cnt(mL[u]);
                    if (rank < m) jj[u] = (int)rpos[rank];
                }
            }
#pragma unroll
            for (int u = 0; u < kSubK; ++u) if (jj[u] >= 0) vj[u] = a[jj[u]];        // (after lane 0's two stores: a partner at m3 reads e0 there)
#pragma unroll
            for (int u = 0; u < kSubK; ++u) if (jj[u] >= 0) { a[p0 + (u << 6) + lane] = vj[u]; a[jj[u]] = e[u]; }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            // children: the smaller one is continued, the larger waits (parts of at most 16 entries are the final insertion sort's; a right part below the skip key is left alone)
            --depth;
            const int nl = cut - first, nr = pk >= skip_key ? last - cut : 0;
            const bool goL = nl > 16, goR = nr > 16;
            if (goL && goR) {
                const bool left_waits = nl >= nr;
                const int wf = left_waits ? first : cut, wn = left_waits ? nl : nr;
                if (sp >= 5) { if (lane == 0) ctl->overflow = 6; sp = 0; last = first; break; }   // (cannot happen: a waiting part is at least twice the part below it)
                st4 = st3; st3 = st2; st2 = st1; st1 = st0; st0 = (uint32_t)wf | ((uint32_t)(wn - 1) << 16) | ((uint32_t)depth << 24); ++sp;
                if (left_waits) first = cut; else last = cut;
            } else if (goL) last = cut;
            else if (goR) first = cut;
            else break;
        }
        if (sp == 0) break;
        --sp;
        first = (int)(st0 & 0xffffu); last = first + (int)((st0 >> 16) & 0xffu) + 1; depth = (int)(st0 >> 24);
        st0 = st1; st1 = st2; st2 = st3; st3 = st4;
    }
    if (prof && lane == 0) { atomicAdd((unsigned long long*)&ctl->t[13], (unsigned long long)(clock64() - ts0)); atomicAdd((unsigned long long*)&ctl->t[14], 1ull); atomicAdd((unsigned long long*)&ctl->t[15], (unsigned long long)nparts); }
}

// ---- queues of the window phase (LDS; lane 0 of a wave, or thread 0, calls these) -----------------------------------------------
__device__ __forceinline__ int lds_add(int* p, int v) { return __hip_atomic_fetch_add(p, v, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ int lds_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP); }

struct SsWin {
    uint32_t* win; lrpos_t* rpos; unsigned long long* q; uint32_t* small; SsCtl* ctl; int* dbg;
    uint32_t skip_key;               // a part whose keys are all below this holds no defined pixel: nothing in it is ever a seed, it is left alone
};
// a child of a partition inside the window: by size to the workgroup's stack, the wave tasks, the list of subtrees a wave finishes alone, or nowhere
__device__ __forceinline__ void route(const SsWin& W, int first, int last, int depth) {
    const int n = last - first;
    if (n <= 16) return;
    if (n <= kSsSub) {                                           // a whole subtree for one wave (wave_sub_sort), after the wave tasks
        const int i = lds_add(&W.ctl->n_small, 1);
        if (i < kSsSmallCap) __hip_atomic_store(&W.small[i], (uint32_t)first | ((uint32_t)(n - 1) << 16) | ((uint32_t)depth << 24), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
        else W.ctl->overflow = 2;
    } else if (n <= kSsTask) {
        lds_add(&W.ctl->q_open, 1);
        const int t = lds_add(&W.ctl->q_tail, 1);
        const unsigned long long rec = (unsigned long long)(uint32_t)first | ((unsigned long long)(uint32_t)last << 16) | ((unsigned long long)(uint32_t)depth << 32) | (1ull << 63);
        __hip_atomic_store(&W.q[t & (kSsQueue - 1)], rec, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
        lds_add(&W.ctl->q_pending, 1);
    } else {
        const int i = W.ctl->w_n;                                // thread 0 only: whole-workgroup phase
        if (i < kSsWStack) { W.ctl->w_first[i] = first; W.ctl->w_last[i] = last; W.ctl->w_depth[i] = depth; W.ctl->w_n = i + 1; }
        else W.ctl->overflow = 3;
    }
}

// The segment ent[gfirst, glast) (17 .. kSsT entries) is finished in LDS.  All threads; starts and ends with barriers.
__device__ __forceinline__ void window_process(uint32_t* ent, int gfirst, int glast, int depth, const SsWin& W, const SsMem& ML) {
    const int tid = threadIdx.x, lane = tid & 63, n = glast - gfirst;
    SsCtl* ctl = W.ctl;
    long long t0 = W.dbg ? clock64() : 0;
    auto lap = [&](int k) { if (W.dbg && tid == 0) { const long long t1 = clock64(); ctl->t[k] += t1 - t0; t0 = t1; } };
    for (int i = tid; i < n; i += kSsThreads) W.win[i] = ent[gfirst + i];
    if (tid == 0) { ctl->w_n = 0; ctl->q_head = ctl->q_tail = ctl->q_pending = ctl->q_open = 0; ctl->n_small = 0; ctl->small_head = 0; }
    for (int i = tid; i < kSsQueue; i += kSsThreads) W.q[i] = 0ull;
    for (int i = tid; i < kSsSmallCap; i += kSsThreads) W.small[i] = 0u;    // a listed subtree's record is never 0: a waiting wave sees its slot filled
    wg_barrier();
    lap(1);
    if (tid == 0) route(W, 0, n, depth);
    while (true) {   // whole-workgroup partitions
        wg_barrier();
        const int sn = uni(ctl->w_n);
        if (sn == 0 || uni(ctl->overflow)) break;                // (overflow: written before this barrier or not at all until the next one -- every wave reads the same)
        const int first = uni(ctl->w_first[sn - 1]), last = uni(ctl->w_last[sn - 1]), d = uni(ctl->w_depth[sn - 1]);
        wg_barrier();
        if (d == 0) {
            if (tid == 0) { libstdcxx::heap_sort(W.win, first, last, KeyDesc()); ctl->w_n = sn - 1; }
            continue;
        }
        const int cut = wg_partition<false>(ML, ctl, first, last, W.skip_key, W.dbg != nullptr);
        if (tid == 0) { ctl->w_n = sn - 1; route(W, first, cut, d - 1); if ((uint32_t)ctl->bc[3] >= W.skip_key) route(W, cut, last, d - 1); }   // right part: keys <= pivot
    }
    lap(2);
    // wave tasks.  The loop is UNIFORM: every lane iterates; lane 0 alone touches the queue counters, in straight-line code whose results
    // are broadcast, and every lane reads the claimed slot itself (same address).  (An earlier version let lane 0 spin in a loop of its own
    // and handed the record over from variables only lane 0 assigned: the compiler let the other lanes leave the task loop on their own
    // and every wave's SECOND partition ran with one lane -- profiles/r04_seed_sort.md.)
    const int wv = uni(tid >> 6);
    // A wave that finds no task to take does not sleep: it holds a TICKET of the list of small subtrees (the next index nobody has taken) and finishes that subtree as
    // soon as its record is there -- the tasks form a tree, so early in a window most waves would wait (45 % busy in round 6's first measurement).  At most one ticket
    // per wave is outstanding; what is still open when the tasks are finished is settled after the barrier below.
    int ticket = -1;
    for (int spins = 0;; ++spins) {
        int st = 0, slot = 0;                                    // 0: nothing to take right now, 1: claimed `slot`, 2: every task is finished
        if (lane == 0) {
            if (lds_load(&ctl->q_open) == 0 || lds_load(&ctl->overflow) != 0) st = 2;   // nothing left -- or the frame has stopped sorting (another wave hit a limit)
            else if (lds_add(&ctl->q_pending, -1) > 0) { slot = lds_add(&ctl->q_head, 1) & (kSsQueue - 1); st = 1; }
            else lds_add(&ctl->q_pending, 1);
        }
        st = __builtin_amdgcn_readfirstlane(st); slot = __builtin_amdgcn_readfirstlane(slot);
        if (st == 2) break;
        if (spins > (1 << 22)) { if (lane == 0) ctl->overflow = 4; break; }   // (a protocol error becomes a status instead of a hang)
        if (st == 0) {
            if (ticket < 0) { int t = 0; if (lane == 0) t = lds_add(&ctl->small_head, 1); ticket = __builtin_amdgcn_readfirstlane(t); }
            uint32_t r = 0;
            if (ticket < kSsSmallCap) r = (uint32_t)__builtin_amdgcn_readfirstlane((int)__hip_atomic_load(&W.small[ticket], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP));
            if (r != 0) {
                const int first = (int)(r & 0xffffu);
                wave_sub_sort(W.win, W.rpos, first, first + (int)((r >> 16) & 0xffu) + 1, (int)(r >> 24), lane, W.skip_key, ctl, W.dbg != nullptr);
                ticket = -1; spins = 0;
            } else __builtin_amdgcn_s_sleep(4);
            continue;
        }
        unsigned rlo = 0, rhi = 0;
        for (int w = 0; w < (1 << 22); ++w) {                    // the pusher holding this ticket writes the slot before it counts the task as pending
            const unsigned long long rec = __hip_atomic_load(&W.q[slot], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP);
            rlo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)rec); rhi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(rec >> 32));
            if (rhi >> 31) break;
            __builtin_amdgcn_s_sleep(1);
        }
        if (!(rhi >> 31)) { if (lane == 0) ctl->overflow = 5; break; }
        if (lane == 0) __hip_atomic_store(&W.q[slot], 0ull, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
        const long long tb = W.dbg ? clock64() : 0;
        // The wave keeps one part of what it has just partitioned for itself (no trip through the queue) while the part is task-sized.
        for (int first = (int)(rlo & 0xffffu), last = (int)(rlo >> 16), d = (int)(rhi & 0xffu);;) {
            if (d == 0) {
                if (lane == 0) libstdcxx::heap_sort(W.win, first, last, KeyDesc());
                break;
            }
            uint32_t pk = 0;
            const int cut = wave_partition(W.win, W.rpos, first, last, d, lane, W.skip_key, &pk);
            if (W.dbg && lane == 0) { const int k = atomicAdd(&W.dbg[1], 1); if (k < 4000) { int* r = W.dbg + 2 + 6 * k; r[0] = wv; r[1] = first; r[2] = last; r[3] = d; r[4] = cut; r[5] = (int)clock(); } }
            if (cut < 0) break;                                  // equal keys: finished
            const bool right_alive = (uint32_t)__builtin_amdgcn_readfirstlane((int)pk) >= W.skip_key;   // right part: keys <= pivot
            --d;
            if (cut - first > kSsSub) {
                if (lane == 0 && right_alive) route(W, cut, last, d);
                last = cut;
            } else if (right_alive && last - cut > kSsSub) {
                if (lane == 0) route(W, first, cut, d);
                first = cut;
            } else {
                if (lane == 0) { route(W, first, cut, d); if (right_alive) route(W, cut, last, d); }
                break;
            }
        }
        if (W.dbg && lane == 0) { const long long dt = clock64() - tb; atomicAdd((unsigned long long*)&ctl->t[8], (unsigned long long)dt); atomicMax((unsigned long long*)&ctl->t[9], (unsigned long long)dt); }
        if (lane == 0) lds_add(&ctl->q_open, -1);
        spins = 0;
    }
    wg_barrier();
    lap(3);
    // subtrees of at most kSsSub entries: a wave takes the next one from the list (they differ in size by a factor of fifteen) and finishes it alone
    const int ns = uni(ctl->overflow) ? 0 : min(uni(ctl->n_small), kSsSmallCap);   // (read after the barrier above; only the stack check of wave_sub_sort writes overflow below)
    while (true) {
        int i = ticket;                                          // (a ticket taken while waiting for tasks comes first)
        ticket = -1;
        if (i < 0) { if (lane == 0) i = lds_add(&ctl->small_head, 1); i = __builtin_amdgcn_readfirstlane(i); }
        if (i >= ns) break;
        const uint32_t r = (uint32_t)__builtin_amdgcn_readfirstlane((int)W.small[i]);
        const int first = (int)(r & 0xffffu);
        wave_sub_sort(W.win, W.rpos, first, first + (int)((r >> 16) & 0xffu) + 1, (int)(r >> 24), lane, W.skip_key, ctl, W.dbg != nullptr);
    }
    wg_barrier();
    lap(4);
    for (int i = tid; i < n; i += kSsThreads) ent[gfirst + i] = W.win[i];
    wg_barrier();
    lap(5);
    if (W.dbg && tid == 0) ctl->t[6] += 1;
}

// std::__introsort_loop(ent, ent + n, depth) by the workgroup.  ws: the frame's scratch (partner positions, chunk masks).
__device__ __forceinline__ void seed_introsort_loop(uint32_t* ent, int n, int depth, uint32_t skip_key, uint32_t* ws, unsigned char* lds, int32_t* status, int* dbg = nullptr) {
    const int tid = threadIdx.x;
    SsCtl* ctl = (SsCtl*)(lds + kOffCtl);
    SsWin W{(uint32_t*)(lds + kOffWin), (lrpos_t*)(lds + kOffRpos), (unsigned long long*)(lds + kOffQ), (uint32_t*)(lds + kOffSmall), ctl, dbg, skip_key};
    const SsMem ML{W.win, W.rpos, (unsigned long long*)(lds + kOffML), (unsigned long long*)(lds + kOffMR), (uint32_t*)(lds + kOffPA), (uint32_t*)(lds + kOffPBx), (uint32_t*)(lds + kOffPBi), 0};
    const int nchg = (n + 63) / 64 + 1;
    // the frame's scratch (seed_sort_ws_entries): word 0 = n_live (out), then the chunk masks of a partition that does not hold them in LDS
    unsigned long long* g_mL = (unsigned long long*)(ws + 2);
    const size_t lds_total = kSsLdsBytes > kOffRpos + 12 * ((size_t)(n + 63) / 64 + 1) + 16 ? kSsLdsBytes : kOffRpos + 12 * ((size_t)(n + 63) / 64 + 1) + 16;   // = lds_bytes(n) below: what the launch asked for
    const SsMem MG{ent, nullptr, g_mL, g_mL + nchg, (uint32_t*)(lds + kOffRpos), nullptr, nullptr, lds_total - kOffRpos - 16};
    if (tid == 0) { ctl->g_n = 1; ctl->g_first[0] = 0; ctl->g_last[0] = n; ctl->g_depth[0] = depth; ctl->overflow = 0; ctl->n_live = n; for (int k = 0; k < 24; ++k) ctl->t[k] = 0; }
    while (true) {
        ss_barrier<true>();                                      // (the entries: built, or moved by the last partition / window, by all waves)
        const int sn = uni(ctl->g_n);
        if (sn == 0) break;
        // (ADVICE r05) a frame that hit a limit or a damaged partition STOPS sorting here: no later stage runs on a segment whose invariants no longer hold.  The
        // entries are still a permutation of the frame's pixels (a skipped swap moves nothing), so the counting sort after this kernel yields every seed once --
        // in an order that is not std::sort's, which status bit 32 tells the caller (plp_line_last_batch_status -> PLP_ERR_OVERFLOW).
        if (uni(ctl->overflow)) break;
        const int first = uni(ctl->g_first[sn - 1]), last = uni(ctl->g_last[sn - 1]), d = uni(ctl->g_depth[sn - 1]);
        wg_barrier();
        if (tid == 0) ctl->g_n = sn - 1;
        if (last - first <= 16) continue;
        if (last - first <= kSsT) { window_process(ent, first, last, d, W, ML); continue; }
        if (d == 0) {
            if (tid == 0) libstdcxx::heap_sort(ent, first, last, KeyDesc());
            continue;
        }
        const long long tg = dbg ? clock64() : 0;
        // two instantiations, so that the masks' address space is known at compile time (LDS instructions, not flat ones)
        bool lm = false;
        const int tile = uni(ss_tile_plan(last - first, MG.lds_bytes_g, &lm));
        if (tile < 1) { if (tid == 0) ctl->overflow = 10; continue; }   // (cannot happen: ss_tile_plan's assertion; the frame stops sorting instead of writing outside its LDS)
        const int cut = lm ? wg_partition<true, true>(MG, ctl, first, last, skip_key, dbg != nullptr, tile) : wg_partition<true, false>(MG, ctl, first, last, skip_key, dbg != nullptr, tile);
        if (dbg && tid == 0) { ctl->t[0] += clock64() - tg; ctl->t[7] += 1; }
        if (tid == 0) {
            int i = ctl->g_n;
            if (i + 2 <= kSsGStack) {
                ctl->g_first[i] = first; ctl->g_last[i] = cut; ctl->g_depth[i] = d - 1; ++i;
                if ((uint32_t)ctl->bc[3] >= skip_key) { ctl->g_first[i] = cut; ctl->g_last[i] = last; ctl->g_depth[i] = d - 1; ++i; }
                ctl->g_n = i;
            } else ctl->overflow = 8;
        }
    }
    // status word 1: WHY the first reporting frame stopped (1 a partition's swap count or cut failed its check, 2 list of small subtrees full, 3 stack of workgroup
    // partitions full, 4 a wave waited for a task beyond the limit, 5 a claimed queue slot stayed empty, 6 / 7 a wave's own stack, 8 stack of global segments, 10 no room for an exchange tile), word 2: that frame
    if (tid == 0) { ws[0] = (uint32_t)(ctl->overflow ? n : ctl->n_live); if (ctl->overflow) { if (atomicOr(status, 32) & 32) {} else { status[1] = ctl->overflow; status[2] = (int32_t)blockIdx.x; status[3] = ctl->overflow == 9 ? ctl->bc[7] : ctl->bc[6]; } } }   // (a frame that stopped sorting: every entry is still there exactly once only over the whole array)
    if (dbg && tid == 0) for (int k = 0; k < 24; ++k) { dbg[2 + 6 * 4000 + 2 * k] = (int)(ctl->t[k] & 0xffffffff); dbg[2 + 6 * 4000 + 2 * k + 1] = (int)(ctl->t[k] >> 32); }
}


// lds bytes for a frame whose seed array has nv entries
inline size_t lds_bytes(size_t nv) { return std::max(kSsLdsBytes, kOffRpos + 12 * ((nv + 63) / 64 + 1) + 16); }

// The frame's seed array: every pixel (x < sw - 1, y < sh - 1) row-major with its gradient bin (lsd.cpp ll_angle), then the
// introsort loop.  P.g2 holds gx^2 + gy^2 of EVERY such pixel in this mode (LsdParams::seed_exact).
__global__ __launch_bounds__(kSsThreads, SS_MINW) void k_lsd_seed_sort(LinePlanes P, LsdParams lp, int n_grad_blocks, uint32_t* ent_all, uint32_t* ws_all, size_t ws_stride) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ss_lds[];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = uni(tid >> 6);
    const int n = P.sw * P.sh, nv = (P.sw - 1) * (P.sh - 1);
    SsCtl* ctl = (SsCtl*)(ss_lds + kOffCtl);
    uint32_t mx = 0;
    for (int i = tid; i < n_grad_blocks; i += kSsThreads) mx = max(mx, P.blockmax[(size_t)b * n_grad_blocks + i]);
    mx = (uint32_t)wave_max((int)mx);
    if (lane == 0) ctl->wsum[0][wv] = (int)mx;
    wg_barrier();
    mx = 0;
    for (int w = 0; w < kSsWaves; ++w) mx = max(mx, (uint32_t)ctl->wsum[0][w]);
    wg_barrier();
    const double max_grad = mx ? sqrt((double)mx / 4.0) : -1.0;
    const double bin_coef = (max_grad > 0) ? (double)(lp.n_bins - 1) / max_grad : 0;
    const uint32_t* g2 = P.g2 + (size_t)b * n;
    uint32_t* ent = ent_all + (size_t)b * nv;
    for (int y = wv; y < P.sh - 1; y += kSsWaves)
        for (int x = lane; x < P.sw - 1; x += 64) {
            const uint32_t pix = (uint32_t)(y * P.sw + x), v = g2[pix];
            const uint32_t bin = (uint32_t)(int)(sqrt((double)v / 4.0) * bin_coef);
            ent[y * (P.sw - 1) + x] = pix | (v >= lp.g2_def_min ? kSsDefBit : 0u) | (bin << kSsShift);
        }
    int lg = 0;
    while ((2 << lg) <= nv) ++lg;
    // Undefined pixels are sorted with the rest (they take part in every partition) but are never seeds: a part that can hold only them
    // -- every key below the bin of the smallest defined magnitude -- is left as it is (70 % of a frame)
    const uint32_t skip_key = (uint32_t)(int)(sqrt((double)lp.g2_def_min / 4.0) * bin_coef);
    seed_introsort_loop(ent, nv, 2 * lg, skip_key, ws_all + (size_t)b * ws_stride, ss_lds, P.status);
}

// test entry: the introsort loop on caller-made entries with a chosen recursion budget
// (copies > 1: diagnostic -- every workgroup sorts its own copy of the entries, so that workgroup 0's phase clocks are taken with the chip as full as in a batch)
__global__ __launch_bounds__(kSsThreads, SS_MINW) void k_seed_sort_debug(uint32_t* ent, int n, int depth, uint32_t skip_key, uint32_t* ws, size_t ws_stride, int32_t* status, int* dbg) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ss_lds[];
    const int b = blockIdx.x;
    if (n > 16) seed_introsort_loop(ent + (size_t)b * n, n, depth, skip_key, ws + (size_t)b * ws_stride, ss_lds, status, b == 0 ? dbg : nullptr);
}

}  // namespace SS_NS
