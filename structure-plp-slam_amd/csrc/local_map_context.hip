// Host driver + C ABI of the matcher context: the local map: module::local_map_updater (include/plp_front.h: plp_local_map_*; local_map_kernels.hip, local_map.hpp)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "matcher_context.hpp"
#include "local_map.hpp"

using namespace plp;

extern "C" {

namespace {
// host: the arrays are host memory, so the two offset tables are checked as well
plp_status lm_check(const plp_local_map_args* a, bool host) {
    if (!a) return set_error(PLP_ERR_INVALID_ARG, "NULL argument");
    if (a->B < 0 || a->F < 0 || a->C < 0 || a->L < 0 || a->LL < 0 || a->T < 0 || a->cap < 0 || a->lcap < 0 || a->fcap < 0 || a->flcap < 0)
        return set_error(PLP_ERR_INVALID_ARG, "B, F, C, L, LL, T, cap, lcap, fcap and flcap must not be negative");
    if (a->frm_stride < 0 || a->frm_stride_lines < 0 || (a->frm_stride && a->frm_stride < a->fcap) || (a->frm_stride_lines && a->frm_stride_lines < a->flcap))
        return set_error(PLP_ERR_INVALID_ARG, "frm_stride and frm_stride_lines must be 0 or at least fcap and flcap");
    if (a->max_num_local_keyfrms < 0 || a->workspace_bytes < 0) return set_error(PLP_ERR_INVALID_ARG, "max_num_local_keyfrms and workspace_bytes must not be negative");
    if (a->k_cap < 0 || a->m_cap < 0 || a->ml_cap < 0) return set_error(PLP_ERR_INVALID_ARG, "k_cap, m_cap and ml_cap must not be negative");
    if (a->F > kLmMaxKf) return set_error(PLP_ERR_UNSUPPORTED, "more than 8192 key frames: the weights of a frame are an LDS table");
    if (a->cap > kLmMaxSlots || a->lcap > kLmMaxSlots || a->fcap > kLmMaxSlots || a->flcap > kLmMaxSlots)
        return set_error(PLP_ERR_UNSUPPORTED, "more than 8192 slots per row");
    if (a->B > kLmMaxFrames) return set_error(PLP_ERR_UNSUPPORTED, "more than 65535 frames");
    if ((long long)a->k_cap * std::max(a->cap, a->lcap) >= (1ll << 31)) return set_error(PLP_ERR_UNSUPPORTED, "k_cap * max(cap, lcap) must stay below 2^31");
    if (a->B == 0) return PLP_OK;
    const bool lines = a->kf_lm_lines != nullptr;
    if (!a->kf_covis && a->F > 0) return set_error(PLP_ERR_INVALID_ARG, "kf_covis is required");
    if (!a->kf_parent && a->F > 0) return set_error(PLP_ERR_INVALID_ARG, "kf_parent is required");
    if (!a->kf_children_offsets || (a->C > 0 && !a->kf_children)) return set_error(PLP_ERR_INVALID_ARG, "kf_children_offsets and kf_children are required");
    if (a->F > 0 && a->cap > 0 && !a->kf_lm) return set_error(PLP_ERR_INVALID_ARG, "kf_lm is required");
    if (!a->obs_offsets || (a->T > 0 && !a->obs_kf)) return set_error(PLP_ERR_INVALID_ARG, "obs_offsets and obs_kf are required");
    if (a->fcap > 0 && !a->frm_lm) return set_error(PLP_ERR_INVALID_ARG, "frm_lm is required");
    if (!a->out_status || !a->out_num_first || !a->out_num_kf || !a->out_nearest_kf || !a->out_num_lm || (a->k_cap > 0 && !a->out_local_kf) ||
        (a->m_cap > 0 && (!a->out_local_lm || !a->out_held)))
        return set_error(PLP_ERR_INVALID_ARG, "out_status, out_num_first, out_num_kf, out_local_kf, out_nearest_kf, out_num_lm, out_local_lm, out_held are required");
    if (lines && (!a->out_num_lines || (a->ml_cap > 0 && (!a->out_local_lines || !a->out_held_lines))))
        return set_error(PLP_ERR_INVALID_ARG, "out_num_lines, out_local_lines, out_held_lines are required with kf_lm_lines");
    if (host) {
        if (a->obs_offsets[0] != 0 || a->obs_offsets[a->L] != a->T) return set_error(PLP_ERR_INVALID_ARG, "obs_offsets must rise from 0 to T");
        for (int l = 0; l < a->L; ++l)
            if (a->obs_offsets[l + 1] < a->obs_offsets[l]) return set_error(PLP_ERR_INVALID_ARG, "obs_offsets must rise from 0 to T");
        if (a->kf_children_offsets[0] != 0 || a->kf_children_offsets[a->F] != a->C) return set_error(PLP_ERR_INVALID_ARG, "kf_children_offsets must rise from 0 to C");
        for (int f = 0; f < a->F; ++f)
            if (a->kf_children_offsets[f + 1] < a->kf_children_offsets[f]) return set_error(PLP_ERR_INVALID_ARG, "kf_children_offsets must rise from 0 to C");
    }
    return PLP_OK;
}

LmArgs lm_args(const plp_local_map_args* a) {
    LmArgs A{};
    A.lines = a->kf_lm_lines != nullptr;
    A.B = a->B; A.F = a->F; A.C = a->C; A.L = a->L; A.LL = A.lines ? a->LL : 0; A.T = a->T; A.cap = a->cap; A.lcap = a->lcap; A.fcap = a->fcap; A.flcap = a->flcap;
    A.frm_stride = a->frm_stride ? a->frm_stride : a->fcap; A.frm_stride_lines = a->frm_stride_lines ? a->frm_stride_lines : a->flcap;
    A.max_kf = a->max_num_local_keyfrms; A.k_cap = a->k_cap; A.m_cap = a->m_cap; A.ml_cap = a->ml_cap;
    A.kf_erased = a->kf_erased; A.kf_covis = a->kf_covis; A.kf_parent = a->kf_parent; A.kf_children_offsets = a->kf_children_offsets; A.kf_children = a->kf_children;
    A.kf_lm = a->kf_lm; A.kf_counts = a->kf_counts; A.kf_lm_lines = a->kf_lm_lines; A.kf_kl_counts = a->kf_kl_counts;
    A.obs_offsets = a->obs_offsets; A.obs_kf = a->obs_kf; A.lm_erased = a->lm_erased; A.lm_erased_lines = a->lm_erased_lines;
    A.frm_lm = a->frm_lm; A.frm_counts = a->frm_counts; A.frm_lm_lines = a->frm_lm_lines; A.frm_kl_counts = a->frm_kl_counts;
    A.out_status = a->out_status; A.out_num_first = a->out_num_first; A.out_num_kf = a->out_num_kf; A.out_local_kf = a->out_local_kf;
    A.out_first_weight = a->out_first_weight; A.out_nearest_kf = a->out_nearest_kf; A.out_num_lm = a->out_num_lm; A.out_local_lm = a->out_local_lm;
    A.out_held = a->out_held; A.out_num_lines = a->out_num_lines; A.out_local_lines = a->out_local_lines; A.out_held_lines = a->out_held_lines;
    A.ws_rows = lm_ws_rows(A.L, A.LL); A.ws_words = lm_ws_words(A.L, A.LL);
    return A;
}

// frames per chunk: as many mark-table rows as fit workspace_bytes, at least one
int lm_chunk(const plp_local_map_args* a, const LmArgs& A) {
    const size_t per = lm_ws_frame_bytes(A.L, A.LL);
    const size_t room = a->workspace_bytes ? (size_t)a->workspace_bytes : (size_t)kLmDefaultWorkspace;
    const size_t n = per ? std::max<size_t>(room / per, 1) : (size_t)A.B;
    return (int)std::min<size_t>(n, (size_t)A.B);
}

// the arrays of a call that works in chunks of nc frames; the room is the mark table of a chunk (lm_ws_frame_bytes is a multiple of 4), 32-bit words
extern "C++" auto lm_plan(int nc) {
    return [nc](auto& r, plp_matcher* c, LmArgs& A) {
        const size_t B = (size_t)A.B, F = (size_t)A.F;
        r.in(A.kf_erased, F); r.in(A.kf_covis, F * kLmCovis); r.in(A.kf_parent, F); r.in(A.kf_children_offsets, F + 1); r.in(A.kf_children, (size_t)A.C);
        r.in(A.kf_lm, F * A.cap); r.in(A.kf_counts, F); r.in(A.kf_lm_lines, F * A.lcap); r.in(A.kf_kl_counts, F);
        r.in(A.obs_offsets, (size_t)A.L + 1); r.in(A.obs_kf, (size_t)A.T); r.in(A.lm_erased, (size_t)A.L); r.in(A.lm_erased_lines, (size_t)A.LL);
        r.in(A.frm_lm, B * A.frm_stride); r.in(A.frm_counts, B); r.in(A.frm_lm_lines, B * A.frm_stride_lines); r.in(A.frm_kl_counts, B);
        r.out(A.out_status, B); r.out(A.out_num_first, B); r.out(A.out_num_kf, B); r.out(A.out_local_kf, B * A.k_cap); r.out(A.out_first_weight, B * A.k_cap);
        r.out(A.out_nearest_kf, B); r.out(A.out_num_lm, B); r.out(A.out_local_lm, B * A.m_cap); r.out(A.out_held, B * A.m_cap);
        if (A.lines) { r.out(A.out_num_lines, B); r.out(A.out_local_lines, B * A.ml_cap); r.out(A.out_held_lines, B * A.ml_cap); }
        r.room(c->lm_ws, A.ws, (size_t)nc * lm_ws_frame_bytes(A.L, A.LL) / 4);
    };
}

// every launch of a call; A.ws holds nc frames
hipError_t lm_run_device(hipStream_t st, LmArgs A, int nc) {
    hipError_t e = launch_local_map_keyframes(st, A);
    for (int b0 = 0; b0 < A.B && e == hipSuccess; b0 += nc) {
        A.b0 = b0; A.nb = std::min(nc, A.B - b0);
        e = launch_local_map_lists(st, A, false);
        if (A.lines && e == hipSuccess) e = launch_local_map_lists(st, A, true);
    }
    return e;
}
}  // namespace

plp_status plp_local_map_device(plp_matcher* c, const plp_local_map_args* a, void* hip_stream) {
    if (!c) return set_error(PLP_ERR_INVALID_ARG, "ctx is NULL");
    if (plp_status s = lm_check(a, false)) return s;
    if (a->B == 0) return PLP_OK;
    const LmArgs A = lm_args(a);
    const int nc = lm_chunk(a, A);
    return device_call(c, hip_stream, A, lm_plan(nc), [nc](hipStream_t st, LmArgs& A) { return lm_run_device(st, A, nc); });
}

plp_status plp_local_map_host(plp_matcher* c, const plp_local_map_args* a) {
    if (!c) return set_error(PLP_ERR_INVALID_ARG, "ctx is NULL");
    if (plp_status s = lm_check(a, true)) return s;
    if (a->B == 0) return PLP_OK;
    const LmArgs A = lm_args(a);
    const int nc = lm_chunk(a, A);
    return host_call(c, A, lm_plan(nc), [nc](hipStream_t st, LmArgs& A) { return lm_run_device(st, A, nc); });
}

// the host build of local_map.hpp (no HIP call): one frame's mark table at a time
int32_t plp_model_local_map_host(const plp_local_map_args* a) {
    if (plp_status s = lm_check(a, true)) return -(int32_t)s;
    LmArgs A = lm_args(a);
    std::vector<uint32_t> ws((size_t)A.ws_rows + A.ws_words + 1);
    std::vector<LmShared> shared(1);
    A.ws = ws.data(); A.nb = 1;
    LmTeamHost par;
    const int kb = lm_mark_blocks(A.k_cap, A.F);
    for (int b = 0; b < A.B; ++b) {
        A.b0 = b;
        lm_keyframes(A, b, shared[0], par);
        for (int side = 0; side < (A.lines ? 2 : 1); ++side) {
            std::fill(ws.begin(), ws.begin() + A.ws_rows, 0xFFFFFFFFu);
            std::fill(ws.begin() + A.ws_rows, ws.end(), 0u);
            LmSharedCompact sc{};
            for (int k = 0; k <= kb; ++k) {
                if (side) lm_mark<true>(A, 0, k, par); else lm_mark<false>(A, 0, k, par);
            }
            if (side) lm_compact<true>(A, 0, sc, par); else lm_compact<false>(A, 0, sc, par);
        }
    }
    return A.B;
}

}  // extern "C"
