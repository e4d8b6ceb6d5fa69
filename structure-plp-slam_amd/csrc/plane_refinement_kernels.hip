// Plane refinement: Planar_Mapping_module::refinement() -- merge_planes, refine_planes, refine_points -- over tables in HBM that are updated in
// place (plp_plane_refinement_*, include/plp_front.h; the reformulation: DESIGN.md section 4).  The semantics are
// plane_refinement.hpp's, which the host build runs as serial loops; the arithmetic of an update is plane_fit.hpp's through a wave as its Team.
//
// Three launches, one per function, one workgroup of four waves per problem in each: workgroup g owns problem g for the whole call and no
// workgroup waits on another.  What a launch leaves for the next stands in the caller's arrays (the tables, out_status, out_num_updates).
// The control flow of a workgroup is uniform (which parent, which candidate, which row is updated next); inside a step the lanes share the work:
//   the candidate loop   for a fixed parent the lanes test 256 candidates at a time and the first that merges is taken.  Whether the
//                        reference's walk tests candidate j (it steps over ONE invalid entry) has a closed form -- a valid j, or an invalid j
//                        at an odd offset into its run of invalid entries counted from where the walk entered -- that a lane reads off the
//                        waves' ballots of the invalid entries; nothing the test reads changes between two merges;
//   Plane::merge         the parent's members are marked in a byte table in HBM, other's entries are compacted by ballot and prefix in slot
//                        order; the count comes first, so that a merge that would pass n_cap writes nothing;
//   an update            D19's steps: compaction of the eligible and the non-erased slots, hypotheses dealt to the four waves (records
//                        through HBM), the replay by every lane, step [4] as a compaction of the members, the ownership writes;
//   refine_points        planes one after the other, members one per lane.
// Data that goes from wave to wave through HBM inside a launch -- hypothesis records, marks, lm_owner, pl_lm, pl_count, pl_equation, pos_w
// between planes -- is handed over by wg_handover(): a workgroup-scope release, the barrier with the stores sent, a workgroup-scope acquire
// (valid without threadgroup split only: the build's -mno-tgsplit).  Tables in LDS are handed over by wg_barrier().
// The loop state that has to outlive an update (which parent, where its walk stands, the counters) is kept in LDS (ctl) and read back behind
// it, and so is the kernel's argument block (PLP_REF_ARGS_IN_LDS): the hypotheses of an update hold the scalar registers of a whole D19 problem,
// and whatever is held across them is spilled to vector lanes (146 spilled SGPRs as one kernel with its state in registers; 2, 0 and 0 now).
#include <hip/hip_runtime.h>

#include "plane_refinement.hpp"
#include "plane_team.hpp"
#include "plp_barrier.hpp"

namespace plp {
namespace {

constexpr int kRefWaves = 4;
constexpr int kNone = 0x7fffffff;

__device__ __forceinline__ void wg_handover() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    wg_barrier_after_global_stores();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// the number of set bits at the top of m
__device__ __forceinline__ int leading_ones(unsigned long long m) { return ~m ? (int)__clzll((long long)~m) : 64; }

// the LDS tables of a workgroup
struct RefLds {
    int32_t* lm;                                          // kPlaneMaxSlots: the list an update or a merge works on
    uint8_t* flag;                                        // kPlaneMaxSlots
    uint16_t* elig;                                       // kPlaneMaxSlots: eligible slots by rank; the members of step [4]; the fresh entries of a merge
    uint16_t* live;                                       // kPlaneMaxSlots
    double* pool;                                         // kPlaneMaxSlots: the waves' inlier lists (4 x 8192 u16); after the hypotheses residuals, errors, gates
    double* work;                                         // kRefWaves x kPlaneWorkDoubles
    uint8_t* state;                                       // kPlaneRefMaxRows: pl_state of the problem, written through
    int* wave_n;                                          // 2 x kRefWaves
    unsigned long long* mask;                             // kRefWaves
};
#define PLP_REF_UPDATE_LDS                                                                                                                  \
    __shared__ int32_t s_lm[kPlaneMaxSlots]; __shared__ uint8_t s_flag[kPlaneMaxSlots]; __shared__ uint16_t s_elig[kPlaneMaxSlots];          \
    __shared__ uint16_t s_live[kPlaneMaxSlots]; __shared__ double s_pool[kPlaneMaxSlots]; __shared__ double s_work[kRefWaves * kPlaneWorkDoubles]; \
    __shared__ uint8_t s_state[kPlaneRefMaxRows]; __shared__ int s_wave_n[2 * kRefWaves]; __shared__ unsigned long long s_mask[kRefWaves];   \
    __shared__ int s_ctl[8];                                                                                                                \
    const RefLds S{s_lm, s_flag, s_elig, s_live, s_pool, s_work, s_state, s_wave_n, s_mask}
// the argument block K of the kernel, copied to LDS as A: what is read from A costs no scalar register between its uses
#define PLP_REF_ARGS_IN_LDS                                                                                                                 \
    __shared__ PlaneRefArgs s_args;                                                                                                         \
    if (threadIdx.x == 0) s_args = K;                                                                                                       \
    wg_barrier()
// ... read where a stretch of code begins: its values live as long as the stretch
#define PLP_REF_ARGS                                                                                                                        \
    const PlaneRefArgs A = args_from_lds(s_args);                                                                                           \
    const RefWho W = ref_who(A)

// a value every lane holds alike, said to the compiler: loops and branches on it are scalar
__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }

// A pointer read back from LDS has lost its address space; every pointer of the argument block is global memory.  (Through an integer: a
// cast from the generic pointer itself is folded away before the address spaces are inferred, and the accesses would be FLAT.)
template <class T> __device__ __forceinline__ T* as_global(T* p) { return (T*)(__attribute__((address_space(1))) T*)(unsigned long long)p; }
__device__ __forceinline__ PlaneRefArgs args_from_lds(const PlaneRefArgs& s) {
    PlaneRefArgs A = s;
    A.G = uni(s.G); A.NP_cap = uni(s.NP_cap); A.n_cap = uni(s.n_cap); A.L = uni(s.L); A.merge_cap = uni(s.merge_cap); A.stages = uni(s.stages);
    A.points_per_ransac = uni(s.points_per_ransac); A.iters = uni(s.iters); A.offset_delta_factor = uni(s.offset_delta_factor);
    A.pl_state = as_global(s.pl_state); A.pl_equation = as_global(s.pl_equation); A.pl_best_error = as_global(s.pl_best_error);
    A.pl_count = as_global(s.pl_count); A.pl_lm = as_global(s.pl_lm); A.pos_w = as_global(s.pos_w); A.lm_erased = as_global(s.lm_erased);
    A.lm_owner = as_global(s.lm_owner); A.dist_thresh = as_global(s.dist_thresh); A.error_thresh = as_global(s.error_thresh);
    A.out_status = as_global(s.out_status); A.out_was_merged = as_global(s.out_was_merged); A.out_planes_changed = as_global(s.out_planes_changed);
    A.out_points_changed = as_global(s.out_points_changed); A.out_removed = as_global(s.out_removed); A.out_num_merges = as_global(s.out_num_merges);
    A.out_merges = as_global(s.out_merges); A.out_num_updates = as_global(s.out_num_updates); A.out_update_status = as_global(s.out_update_status);
    A.out_lm_changed = as_global(s.out_lm_changed); A.ctx_hyp = as_global(s.ctx_hyp); A.ctx_mark = as_global(s.ctx_mark);
    return A;
}

// who a thread is
struct RefWho {
    int g, tid, lane, w;
    size_t pbase, lbase;
    unsigned long long below;
};
__device__ __forceinline__ RefWho ref_who(const PlaneRefArgs& A) {
    RefWho W;
    W.g = blockIdx.x; W.tid = threadIdx.x; W.lane = W.tid & 63; W.w = __builtin_amdgcn_readfirstlane(W.tid >> 6);
    W.pbase = (size_t)W.g * A.NP_cap; W.lbase = (size_t)W.g * A.L;
    W.below = (1ull << W.lane) - 1ull;
    return W;
}

__device__ __forceinline__ int ctl_get(const int* ctl, int k) { return uni(ctl[k]); }

// the ranks of two predicates among the workgroup's 256 lanes, and their totals (uniform call)
__device__ __forceinline__ int rank2(const RefLds& S, const RefWho& W, bool p0, bool p1, int& tot0, int& tot1, int& r1) {
    const unsigned long long m0 = __ballot(p0), m1 = __ballot(p1);
    if (W.lane == 0) { S.wave_n[W.w] = (int)__popcll(m0); S.wave_n[kRefWaves + W.w] = (int)__popcll(m1); }
    wg_barrier();
    int o0 = 0, o1 = 0;
    tot0 = 0; tot1 = 0;
#pragma unroll
    for (int u = 0; u < kRefWaves; ++u) {
        if (u < W.w) { o0 += S.wave_n[u]; o1 += S.wave_n[kRefWaves + u]; }
        tot0 += S.wave_n[u]; tot1 += S.wave_n[kRefWaves + u];
    }
    wg_barrier();                                         // wave_n is rewritten by the next call
    tot0 = uni(tot0); tot1 = uni(tot1);
    r1 = o1 + (int)__popcll(m1 & W.below);
    return o0 + (int)__popcll(m0 & W.below);
}
__device__ __forceinline__ int rank1(const RefLds& S, const RefWho& W, bool p, int& tot) {
    int t1, r1;
    return rank2(S, W, p, false, tot, t1, r1);
}

__device__ __forceinline__ void set_state(const PlaneRefArgs& A, const RefLds& S, const RefWho& W, int row, uint8_t st) {   // one lane; a barrier follows
    S.state[row] = st;
    A.pl_state[W.pbase + row] = st;
}

// pl_state to LDS; the rows with IN_DB compacted in ascending row into rows (NULL: not wanted).  Returns their number.
__device__ __forceinline__ int load_state(const PlaneRefArgs& A, const RefLds& S, const RefWho& W, uint16_t* rows) {
    int n_db = 0;
    for (int base = 0; base < A.NP_cap; base += 256) {
        const int r = base + W.tid;
        uint8_t st = 0;
        if (r < A.NP_cap) { st = A.pl_state[W.pbase + r]; S.state[r] = st; }
        const bool in = (st & PLP_PLANE_ROW_IN_DB) != 0;
        int tot;
        const int k = rank1(S, W, in, tot);
        if (in && rows) rows[n_db + k] = (uint16_t)r;
        n_db += tot;
    }
    wg_barrier();
    return n_db;
}

// update_plane_via_RANSAC (:593-733) of `row`, the c-th update call of the problem (uniform calls), in two halves.  The first, up to the
// hypotheses' records, reads the kernel's own argument block: it is the half that needs the scalar registers.  Returns where the function
// returns before its loop (the state byte is then written), else PLP_PLANE_OK.
__device__ __forceinline__ int update_hypotheses(const PlaneRefArgs& A, const RefLds& S, int row, int c) {
    const RefWho W = ref_who(A);
    const int tid = W.tid, lane = W.lane, w = W.w, I = A.iters;
    const size_t prow = W.pbase + row, lbase = W.lbase;
    const int n = uni(clamp_count(A.pl_count, (int)prow, A.n_cap));
    const int32_t* lst = A.pl_lm + prow * A.n_cap;
    const double* pos = A.pos_w + 3 * lbase;
    const double thr = A.dist_thresh[W.g];
    const PlaneArgs U = plane_update_args(A);
    double* const hyp = A.ctx_hyp + (size_t)W.g * I * kPlaneHypDoubles;
    int n_elig = 0, n_live = 0;
    for (int base = 0; base < n; base += 256) {
        const int slot = base + tid;
        uint8_t f = (uint8_t)PLP_PLANE_LM_ERASED;
        if (slot < n) {
            const int lm = lst[slot];
            f = plane_slot_flag(A, lbase, lm);
            S.lm[slot] = lm; S.flag[slot] = f;
        }
        const bool e = slot < n && plane_eligible(PLP_PLANE_UPDATE, f), l = slot < n && plane_live(f);
        int te, tl, rl;
        const int re = rank2(S, W, e, l, te, tl, rl);
        if (e) S.elig[n_elig + re] = (uint16_t)slot;
        if (l) S.live[n_live + rl] = (uint16_t)slot;
        n_elig += te; n_live += tl;
    }
    wg_barrier();                                         // the lists
    int flags = 0;
    const int early = plane_early_status(U, n, n_elig, flags);
    if (early != PLP_PLANE_OK) {                          // uniform
        if (tid == 0) {
            A.out_update_status[prow] = (uint8_t)early;
            set_state(A, S, W, row, plane_state_after_update(S.state[row], flags));
        }
        wg_barrier();
        return early;
    }
    const int m = plane_sample_size(PLP_PLANE_UPDATE, n, A.points_per_ransac);
    const unsigned long long seed = A.seed + (unsigned long long)W.g;
    {
        PlaneWaveTeam T{lane, S.work + w * kPlaneWorkDoubles};
        uint16_t* list = reinterpret_cast<uint16_t*>(S.pool) + (size_t)w * kPlaneMaxSlots;
        for (int it = w; it < I; it += kRefWaves) {
            double eq_s[4], res;
            int sweeps;
            plane_fit(T, [&](int k, double x[3]) {
                const int rank = ransac_draw_one(seed, c, it, k, n_elig);
                if ((unsigned)rank >= (unsigned)n_elig) return false;
                const double* q = pos + 3 * (size_t)S.lm[S.elig[rank]];
                x[0] = q[0]; x[1] = q[1]; x[2] = q[2];
                return true;
            }, m, eq_s, res, sweeps);
            const double abs_n = plane_abs_n(eq_s);
            int cnt = 0;
            for (int base = 0; base < n_live; base += 64) {   // step [2]: the inliers in slot order
                const int r = base + lane;
                bool in = false;
                int slot = 0;
                if (r < n_live) {
                    slot = S.live[r];
                    const double* q = pos + 3 * (size_t)S.lm[slot];
                    const double x[3] = {q[0], q[1], q[2]};
                    in = plane_distance(eq_s, abs_n, x) < thr;
                }
                const unsigned long long mk = __ballot(in);
                if (in) list[cnt + (int)__popcll(mk & W.below)] = (uint16_t)slot;
                cnt += (int)__popcll(mk);
            }
            __builtin_amdgcn_wave_barrier();              // the list is read by other lanes of this wave: LDS keeps a wave's order
            const bool tried = plane_refit_gate(U, n, cnt);
            double eq_r[4] = {0.0, 0.0, 0.0, 0.0}, err = kPlaneMax;
            if (tried)                                    // uniform over the wave
                plane_fit(T, [&](int k, double x[3]) {
                    const double* q = pos + 3 * (size_t)S.lm[list[k]];
                    x[0] = q[0]; x[1] = q[1]; x[2] = q[2];
                    return true;
                }, cnt, eq_r, err, sweeps);
            __builtin_amdgcn_wave_barrier();              // the next iteration rewrites the list
            if (lane == 0) {
                double* rec = hyp + (size_t)it * kPlaneHypDoubles;
#pragma unroll
                for (int i = 0; i < 4; ++i) { rec[i] = eq_s[i]; rec[5 + i] = eq_r[i]; }
                rec[4] = res; rec[9] = err; rec[10] = (double)cnt; rec[11] = tried ? 1.0 : 0.0;
            }
        }
    }
    wg_handover();                                        // the records; the waves' lists are dead
    return PLP_PLANE_OK;
}

// ... and the second half, behind the records: the replay, step [4], the tables.  Everything it needs it reads again (A: the block's copy in LDS).
__device__ __forceinline__ int update_finish(const PlaneRefArgs& A, const RefLds& S, const RefWho& W, int row) {
    const int tid = W.tid, I = A.iters, L = A.L;
    const size_t prow = W.pbase + row, lbase = W.lbase;
    const int n = uni(clamp_count(A.pl_count, (int)prow, A.n_cap));
    int32_t* lst = A.pl_lm + prow * A.n_cap;
    const double best_error_in = A.pl_best_error[prow];
    const double* pos = A.pos_w + 3 * lbase;
    const double thr = A.dist_thresh[W.g], error_thresh = A.error_thresh[W.g];
    const double* hyp = A.ctx_hyp + (size_t)W.g * I * kPlaneHypDoubles;
    int flags = 0;
    double* s_res = S.pool;
    double* s_err = S.pool + kPlaneMaxIters;
    uint8_t* s_tried = reinterpret_cast<uint8_t*>(S.pool + 2 * kPlaneMaxIters);
    for (int it = tid; it < I; it += 256) {
        const double* rec = hyp + (size_t)it * kPlaneHypDoubles;
        s_res[it] = rec[4]; s_err[it] = rec[9]; s_tried[it] = rec[11] != 0.0 ? 1 : 0;
    }
    wg_barrier();
    const PlaneReplay R = plane_replay(PLP_PLANE_UPDATE, I, best_error_in, error_thresh, [&](int i) { return s_res[i]; },
                                       [&](int i) { return s_tried[i] != 0; }, [&](int i) { return s_err[i]; });
    int status = plane_late_status(PLP_PLANE_UPDATE, R, error_thresh, flags);
    const double* rec_l = hyp + (size_t)R.last_iter * kPlaneHypDoubles + (R.last_refit ? 5 : 0);
    const double* rec_b = hyp + (size_t)(R.best_iter < 0 ? R.last_iter : R.best_iter) * kPlaneHypDoubles;
    const double eq[4] = {rec_l[0], rec_l[1], rec_l[2], rec_l[3]}, eq_b[4] = {rec_b[0], rec_b[1], rec_b[2], rec_b[3]};
    const double abs_n = plane_abs_n(eq), abs_b = plane_abs_n(eq_b);
    int num = 0;
    if (status == PLP_PLANE_OK) {                         // step [4] (:704-720): the members, compacted in slot order
        for (int base = 0; base < n; base += 256) {
            const int s = base + tid;
            bool in = false;
            if (s < n && plane_live(S.flag[s])) {
                const double* q = pos + 3 * (size_t)S.lm[s];
                const double x[3] = {q[0], q[1], q[2]};
                in = plane_distance(eq_b, abs_b, x) < thr && plane_distance(eq, abs_n, x) < thr;
            }
            int tot;
            const int r = rank1(S, W, in, tot);
            if (in) S.elig[num + r] = (uint16_t)s;
            num += tot;
        }
        if (num < A.points_per_ransac) { status = PLP_PLANE_TOO_FEW_LEFT; flags = PLP_PLANE_FLAG_INVALID; }   // :722
    }
    wg_barrier();                                         // the members; every lane has replayed from the pool
    if (tid == 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) A.pl_equation[4 * prow + i] = eq[i];
        A.pl_best_error[prow] = R.plane_error;
        A.out_update_status[prow] = (uint8_t)status;
        set_state(A, S, W, row, plane_state_after_update(S.state[row], flags));
    }
    if (status == PLP_PLANE_OK) {                         // :728-730
        for (int s = tid; s < n; s += 256) {
            const int lm = S.lm[s];
            if ((unsigned)lm < (unsigned)L) A.lm_owner[lbase + lm] = -1;
        }
        wg_handover();
        for (int k = tid; k < num; k += 256) {
            const int lm = S.lm[S.elig[k]];
            lst[k] = lm;
            A.lm_owner[lbase + lm] = row;
        }
        if (tid == 0) A.pl_count[prow] = num;
    }
    wg_handover();
    return status;
}

// Plane::merge (landmark_plane.cc:221-248) of `other` into `parent` (uniform call): false when the list would pass n_cap, nothing written
__device__ __forceinline__ bool merge(const PlaneRefArgs& A, const RefLds& S, const RefWho& W, int parent, int other) {
    const int tid = W.tid, L = A.L;
    const size_t pbase = W.pbase, lbase = W.lbase;
    uint8_t* const mark = A.ctx_mark + lbase;
    const int np = uni(clamp_count(A.pl_count, (int)(pbase + parent), A.n_cap)), no = uni(clamp_count(A.pl_count, (int)(pbase + other), A.n_cap));
    int32_t* pl = A.pl_lm + (pbase + parent) * A.n_cap;
    const int32_t* ol = A.pl_lm + (pbase + other) * A.n_cap;
    for (int s = tid; s < np; s += 256) {
        const int lm = pl[s];
        if ((unsigned)lm < (unsigned)L) mark[lm] = 1;
    }
    wg_handover();
    int fresh = 0;
    for (int base = 0; base < no; base += 256) {
        const int s = base + tid;
        bool add = false;
        if (s < no) {
            const int lm = ol[s];
            const bool named = (unsigned)lm < (unsigned)L, live = named && A.lm_erased[lbase + lm] == 0;
            S.lm[s] = lm;
            S.flag[s] = (uint8_t)((named ? 1 : 0) | (live ? 2 : 0));
            add = live && mark[lm] == 0;
        }
        int tot;
        const int r = rank1(S, W, add, tot);
        if (add) S.elig[fresh + r] = (uint16_t)s;
        fresh += tot;
    }
    wg_barrier();
    const bool fits = np + fresh <= A.n_cap;
    if (fits) {
        for (int s = tid; s < no; s += 256)
            if (S.flag[s] & 1) A.lm_owner[lbase + S.lm[s]] = -1;                               // remove_landmarks_ownership() (:233)
        wg_handover();
        for (int s = tid; s < no; s += 256)
            if (S.flag[s] & 2) A.lm_owner[lbase + S.lm[s]] = parent;                           // :240
        for (int k = tid; k < fresh; k += 256) pl[np + k] = S.lm[S.elig[k]];                   // :239
        if (tid == 0) {
            A.pl_count[pbase + parent] = np + fresh;
            set_state(A, S, W, parent, (uint8_t)(S.state[parent] | PLP_PLANE_ROW_NEED_REFINEMENT));   // :244
        }
        if (tid == 64) set_state(A, S, W, other, (uint8_t)(S.state[other] & ~PLP_PLANE_ROW_VALID));   // :247
    }
    for (int s = tid; s < np; s += 256) {
        const int lm = pl[s];
        if ((unsigned)lm < (unsigned)L) mark[lm] = 0;
    }
    wg_handover();
    return fits;
}

// the first entry j >= j0 of the compacted vector that the walk of parent `ri` tests and that merges with it, n_db when none (uniform call)
__device__ __forceinline__ int first_merge(const PlaneRefArgs& A, const RefLds& S, const RefWho& W, const uint16_t* rows, int ri, int j0, int n_db,
                                           double offset_thr) {
    const int lane = W.lane, w = W.w;
    const double* pe = A.pl_equation + 4 * (W.pbase + ri);
    const double eq_i[4] = {pe[0], pe[1], pe[2], pe[3]};
    int carry = 0;                                        // invalid entries directly in front of the chunk, back to j0
    for (int base = j0; base < n_db; base += 256) {
        const int j = base + W.tid;
        bool inv = false;
        int rj = 0;
        if (j < n_db) { rj = rows[j]; inv = (S.state[rj] & PLP_PLANE_ROW_VALID) == 0; }
        const unsigned long long mk = __ballot(inv);
        if (lane == 0) S.mask[w] = mk;
        wg_barrier();
        int before;
        const unsigned long long valid_below = ~mk & W.below;
        if (valid_below) {
            before = lane - 1 - (63 - (int)__clzll((long long)valid_below));
        } else {
            before = lane;
            int u = w - 1;
            for (; u >= 0; --u) {
                const int lo = leading_ones(S.mask[u]);
                before += lo;
                if (lo < 64) break;
            }
            if (u < 0) before += carry;
        }
        int next = 0;
        {
            int u = kRefWaves - 1;
            for (; u >= 0; --u) {
                const int lo = leading_ones(S.mask[u]);
                next += lo;
                if (lo < 64) break;
            }
            if (u < 0) next += carry;
        }
        bool hit = false;
        if (j < n_db && plane_candidate_tested(!inv, before)) {
            const double* pj = A.pl_equation + 4 * (W.pbase + rj);
            const double eq_j[4] = {pj[0], pj[1], pj[2], pj[3]};
            hit = plane_pair_test(eq_i, eq_j, offset_thr, A.dot_thr) == kPlanePairMerge;
        }
        const unsigned long long mh = __ballot(hit);
        if (lane == 0) S.wave_n[w] = mh ? base + w * 64 + (int)__builtin_ctzll(mh) : kNone;
        wg_barrier();
        int found = kNone;
#pragma unroll
        for (int u = 0; u < kRefWaves; ++u) found = S.wave_n[u] < found ? S.wave_n[u] : found;
        wg_barrier();                                     // mask and wave_n are rewritten
        found = uni(found);
        if (found != kNone) return found;
        carry = next;
    }
    return n_db;
}

// the slots of ctl
enum { kCtlI = 0, kCtlJ0 = 1, kCtlMerges = 2, kCtlUpdates = 3, kCtlNdb = 4, kCtlChanged = 5 };

// refinement()'s gate (:777), merge_planes (:795-898) and the outputs every call writes
__global__ __launch_bounds__(256) void k_plane_ref_merge(PlaneRefArgs K) {
    PLP_REF_UPDATE_LDS;
    PLP_REF_ARGS_IN_LDS;
    __shared__ uint8_t s_rm[kPlaneRefMaxRows];            // on planes_will_be_removed
    __shared__ uint16_t s_rows[kPlaneRefMaxRows];         // get_all_landmark_planes()
    const int tid = threadIdx.x;
    int status = PLP_PLANE_REFINEMENT_OK;
    bool run = false;
    {
        PLP_REF_ARGS;
        for (int r = tid; r < A.NP_cap; r += 256) {
            s_rm[r] = 0;
            A.out_removed[W.pbase + r] = 0;
            A.out_update_status[W.pbase + r] = (uint8_t)kPlaneRefNoUpdate;
        }
        for (int l = tid; l < A.L; l += 256) {
            A.out_lm_changed[W.lbase + l] = 0;
            A.ctx_mark[W.lbase + l] = 0;
        }
        const int n_db0 = load_state(A, S, W, s_rows);
        if (tid == 0) { s_ctl[kCtlI] = 0; s_ctl[kCtlJ0] = -1; s_ctl[kCtlMerges] = 0; s_ctl[kCtlUpdates] = 0; s_ctl[kCtlNdb] = n_db0; }
        wg_handover();
        if (A.stages == 7 && n_db0 < 2) status = PLP_PLANE_REFINEMENT_TOO_FEW_PLANES;          // :777
        run = status == PLP_PLANE_REFINEMENT_OK && (A.stages & PLP_PLANE_STAGE_MERGE) && n_db0 >= 2;   // :799-808
    }
    while (run) {
        int parent, c;
        {
            PLP_REF_ARGS;
            const int n_db = ctl_get(s_ctl, kCtlNdb);
            int i = ctl_get(s_ctl, kCtlI), j0 = ctl_get(s_ctl, kCtlJ0);
            int jm = n_db, ri = 0;
            for (; i < n_db; ++i, j0 = -1) {              // to the next pair that merges; nothing is written on the way
                ri = uni(s_rows[i]);
                if (j0 < 0) {
                    if ((uni(S.state[ri]) & PLP_PLANE_ROW_VALID) == 0) continue;                 // :820, once per i
                    j0 = i + 1;
                }
                if (j0 < n_db) jm = first_merge(A, S, W, s_rows, ri, j0, n_db, (double)A.offset_delta_factor * A.dist_thresh[W.g]);   // :813
                if (jm < n_db) break;
            }
            if (i >= n_db) break;
            const int rj = uni(s_rows[jm]);
            const int ci = uni(clamp_count(A.pl_count, (int)(W.pbase + ri), A.n_cap)), cj = uni(clamp_count(A.pl_count, (int)(W.pbase + rj), A.n_cap));
            const int other = ci > cj ? rj : ri;                                                // :864
            parent = ci > cj ? ri : rj;
            if (!merge(A, S, W, parent, other)) { status = PLP_PLANE_REFINEMENT_OVERFLOW; break; }
            c = ctl_get(s_ctl, kCtlUpdates);
            wg_barrier();                                 // ctl is read before it is rewritten
            if (tid == 0) {
                const int nm = s_ctl[kCtlMerges];
                s_rm[other] = 1;                                                                // :867, :876
                if (nm < A.merge_cap) {
                    A.out_merges[2 * ((size_t)W.g * A.merge_cap + nm)] = parent;
                    A.out_merges[2 * ((size_t)W.g * A.merge_cap + nm) + 1] = other;
                }
                s_ctl[kCtlI] = i; s_ctl[kCtlJ0] = jm + 1; s_ctl[kCtlMerges] = nm + 1; s_ctl[kCtlUpdates] = c + 1;
                s_ctl[6] = parent;
            }
        }
        const int early = update_hypotheses(K, S, parent, c);                                   // :870, :879
        {
            PLP_REF_ARGS;
            const int p = ctl_get(s_ctl, 6);
            if (early == PLP_PLANE_OK) update_finish(A, S, W, p);
            if (tid == 0) set_state(A, S, W, p, (uint8_t)(S.state[p] | PLP_PLANE_ROW_NEED_REFINEMENT));   // :871, :880
            wg_barrier();
        }
    }
    {
        PLP_REF_ARGS;
        if (run && status == PLP_PLANE_REFINEMENT_OK)
            for (int r = tid; r < A.NP_cap; r += 256)
                if (s_rm[r]) {                                                                  // :889-895
                    set_state(A, S, W, r, (uint8_t)(S.state[r] & ~PLP_PLANE_ROW_IN_DB));
                    A.out_removed[W.pbase + r] = 1;
                }
        if (tid == 0) {
            const int nm = s_ctl[kCtlMerges];
            A.out_status[W.g] = (uint8_t)status;
            A.out_was_merged[W.g] = nm > 0 ? 1 : 0; A.out_planes_changed[W.g] = 0; A.out_points_changed[W.g] = 0;
            A.out_num_merges[W.g] = nm; A.out_num_updates[W.g] = s_ctl[kCtlUpdates];
        }
    }
}

// refine_planes (:900-952)
__global__ __launch_bounds__(256) void k_plane_ref_planes(PlaneRefArgs K) {
    PLP_REF_UPDATE_LDS;
    PLP_REF_ARGS_IN_LDS;
    __shared__ uint8_t s_er[kPlaneRefMaxRows];            // on planes_will_be_erased
    const int tid = threadIdx.x;
    {
        PLP_REF_ARGS;
        if (uni(A.out_status[W.g]) != PLP_PLANE_REFINEMENT_OK) return;                          // uniform
        for (int r = tid; r < A.NP_cap; r += 256) s_er[r] = 0;
        load_state(A, S, W, nullptr);
        if (tid == 0) { s_ctl[kCtlI] = 0; s_ctl[kCtlUpdates] = A.out_num_updates[W.g]; s_ctl[kCtlChanged] = 0; }
        wg_barrier();
    }
    for (;;) {
        int r, c;
        {
            PLP_REF_ARGS;
            r = ctl_get(s_ctl, kCtlI);
            for (; r < A.NP_cap; ++r) {                   // to the next row that is updated
                const int st = uni(S.state[r]);
                if ((st & PLP_PLANE_ROW_IN_DB) == 0) continue;
                if ((st & PLP_PLANE_ROW_VALID) == 0) {                                          // :907-911
                    if (tid == 0) s_er[r] = 1;
                } else if (st & PLP_PLANE_ROW_NEED_REFINEMENT) {
                    break;
                } else if (uni(clamp_count(A.pl_count, (int)(W.pbase + r), A.n_cap)) < 2 * A.points_per_ransac) {
                    if (tid == 0) s_er[r] = 1;                                                  // :926-929
                }
            }
            if (r >= A.NP_cap) break;
            c = ctl_get(s_ctl, kCtlUpdates);
            wg_barrier();                                 // ctl is read before it is rewritten
            if (tid == 0) { s_ctl[kCtlI] = r + 1; s_ctl[kCtlUpdates] = c + 1; s_ctl[6] = r; }
        }
        const int early = update_hypotheses(K, S, r, c);                                        // :917
        {
            PLP_REF_ARGS;
            const int row = ctl_get(s_ctl, 6);
            const bool done = early == PLP_PLANE_OK && update_finish(A, S, W, row) == PLP_PLANE_OK;
            if (done && tid == 0) {
                set_state(A, S, W, row, (uint8_t)(S.state[row] & ~PLP_PLANE_ROW_NEED_REFINEMENT));
                s_ctl[kCtlChanged] = 1;
            }
            wg_barrier();
        }
    }
    wg_barrier();
    PLP_REF_ARGS;
    for (int r = 0; r < A.NP_cap; ++r) {                                                        // :934-941
        if (!uni(s_er[r])) continue;
        const int n = uni(clamp_count(A.pl_count, (int)(W.pbase + r), A.n_cap));
        const int32_t* lst = A.pl_lm + (W.pbase + r) * A.n_cap;
        for (int s = tid; s < n; s += 256) {
            const int lm = lst[s];
            if ((unsigned)lm < (unsigned)A.L) A.lm_owner[W.lbase + lm] = -1;
        }
    }
    for (int r = tid; r < A.NP_cap; r += 256)
        if (s_er[r]) {
            set_state(A, S, W, r, (uint8_t)(S.state[r] & ~PLP_PLANE_ROW_IN_DB));
            A.out_removed[W.pbase + r] = (uint8_t)(A.out_removed[W.pbase + r] | 2);
        }
    if (tid == 0) { A.out_planes_changed[W.g] = (uint8_t)s_ctl[kCtlChanged]; A.out_num_updates[W.g] = s_ctl[kCtlUpdates]; }
}

// refine_points (:954-1004)
__global__ __launch_bounds__(256) void k_plane_ref_points(PlaneRefArgs A) {
    __shared__ int s_any;
    const RefWho W = ref_who(A);
    const int tid = W.tid;
    if (A.out_status[W.g] != PLP_PLANE_REFINEMENT_OK) return;                                   // uniform
    if (tid == 0) s_any = 0;
    wg_barrier();
    const double thr = A.dist_thresh[W.g];
    bool moved = false;
    for (int r = 0; r < A.NP_cap; ++r) {
        const int n = uni(clamp_count(A.pl_count, (int)(W.pbase + r), A.n_cap));
        if (!plane_row_active(A.pl_state[W.pbase + r], n, A.points_per_ransac)) continue;       // :960-965
        const double* pe = A.pl_equation + 4 * (W.pbase + r);
        const double eq[4] = {pe[0], pe[1], pe[2], pe[3]};
        const int32_t* lst = A.pl_lm + (W.pbase + r) * A.n_cap;
        for (int s = tid; s < n; s += 256) {
            const int lm = lst[s];
            const uint8_t f = plane_slot_flag(A, W.lbase, lm);
            if (!plane_live(f) || (f & PLP_PLANE_LM_OWNED) == 0) continue;                      // :970
            double* q = A.pos_w + 3 * (W.lbase + lm);
            double x[3] = {q[0], q[1], q[2]};
            if (plane_refine_point(eq, thr, x)) {
                q[0] = x[0]; q[1] = x[1]; q[2] = x[2];
                A.out_lm_changed[W.lbase + lm] = 1;
                moved = true;
            }
        }
        wg_handover();                                                                          // the next plane may move the same landmarks
    }
    if (moved) s_any = 1;
    wg_barrier();
    if (tid == 0) A.out_points_changed[W.g] = s_any ? 1 : 0;
}

}  // namespace

hipError_t launch_plane_refinement(hipStream_t st, const PlaneRefArgs& A) {
    hipLaunchKernelGGL(k_plane_ref_merge, dim3(A.G), dim3(256), 0, st, A);
    if (A.stages & PLP_PLANE_STAGE_REFINE_PLANES) hipLaunchKernelGGL(k_plane_ref_planes, dim3(A.G), dim3(256), 0, st, A);
    if (A.stages & PLP_PLANE_STAGE_REFINE_POINTS) hipLaunchKernelGGL(k_plane_ref_points, dim3(A.G), dim3(256), 0, st, A);
    return hipGetLastError();
}

}  // namespace plp
