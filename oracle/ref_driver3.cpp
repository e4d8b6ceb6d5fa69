// TEST INFRASTRUCTURE ONLY.  C ABI over the reference's own data/graph_node.cc and module/local_map_cleaner.cc (compiled unmodified by
// oracle/ref_build.sh into oracle/_ref/libplpref3.so) in the table layouts of include/plp_front.h: plp_covisibility_update_args,
// plp_covisibility_erase_args, plp_cull_keyframes_args, plp_cull_landmarks_args.  tests/ref_map_lib.py loads it with ctypes.
//
// What comes from where:
//   the reference's object code   everything in graph_node.cc; the loops, gates, counting and float decisions of local_map_cleaner.cc
//   oracle/ref_shadow_map         the cascade of an erased key frame (keyframe::prepare_for_erasing, landmark::erase_observation,
//                                 landmark::prepare_for_erasing, keyframe::erase_landmark_with_index): restated, not a pin
//   this file                     tables <-> objects.  The key frames of a scene are ONE contiguous array, so ascending pointer is ascending
//                                 row: the correspondence DESIGN.md section 5 (D18, D20, D21) defines for std::map<keyframe*, ...> and
//                                 std::pair<unsigned, keyframe*>.  A row outside its table is no object (D20 item 6, D21 item 1): a slot
//                                 becomes nullptr, an observation no entry, a count is cut to [0, cap]; what was dropped is counted in
//                                 `dropped` = {slots, observations, landmarks whose list names a key frame twice, list entries}.
// This file alone is compiled with -fno-access-control: it presets and reads graph_node's private tables and local_map_cleaner's buffers.
#include <cstdint>
#include <cstring>
#include <list>
#include <memory>
#include <set>
#include <vector>

#include "PLPSLAM/data/keyframe.h"
#include "PLPSLAM/data/landmark.h"
#include "PLPSLAM/data/landmark_line.h"
#include "PLPSLAM/data/graph_node.h"
#include "PLPSLAM/module/local_map_cleaner.h"
#include "plp_front.h"

using namespace PLPSLAM;
using data::keyframe;
using data::landmark;

namespace
{
    struct snapshot
    { // the union of what the two update / cull argument structs say about a map
        int F = 0, L = 0, T = 0, cap = 0, kp_stride = 0;
        const int32_t *kf_lm = nullptr, *kf_counts = nullptr, *obs_offsets = nullptr, *obs_kf = nullptr, *obs_idx = nullptr;
        const plp_keypoint *undist = nullptr;
        const float *x_right = nullptr, *depths = nullptr, *depth_thr = nullptr;
        const uint32_t *kf_id = nullptr, *lm_num_obs = nullptr;
        const uint8_t *kf_erased = nullptr, *kf_cannot_erase = nullptr, *lm_erased = nullptr;
        bool has_origin = false;
        uint32_t origin_id = 0;
    };

    snapshot of(const plp_covisibility_update_args *a)
    {
        snapshot s;
        s.F = a->F, s.L = a->L, s.T = a->T, s.cap = a->cap, s.kp_stride = a->cap;
        s.kf_lm = a->kf_lm, s.kf_counts = a->kf_counts, s.obs_offsets = a->obs_offsets, s.obs_kf = a->obs_kf;
        s.kf_id = a->kf_id, s.lm_erased = a->lm_erased;
        return s;
    }

    snapshot of(const plp_cull_keyframes_args *a)
    {
        snapshot s;
        s.F = a->F, s.L = a->L, s.T = a->T, s.cap = a->cap, s.kp_stride = a->kp_stride ? a->kp_stride : a->cap;
        s.kf_lm = a->kf_lm, s.kf_counts = a->kf_counts, s.obs_offsets = a->obs_offsets, s.obs_kf = a->obs_kf, s.obs_idx = a->obs_idx;
        s.undist = a->undist, s.x_right = a->x_right, s.depths = a->depths, s.depth_thr = a->depth_thr;
        s.kf_id = a->kf_id, s.lm_num_obs = a->lm_num_obs, s.kf_erased = a->kf_erased, s.kf_cannot_erase = a->kf_cannot_erase, s.lm_erased = a->lm_erased;
        s.has_origin = true, s.origin_id = a->origin_id;
        return s;
    }

    struct world
    {
        int F = 0, L = 0;
        std::unique_ptr<keyframe[]> kfs;
        std::unique_ptr<landmark[]> lms;
        int64_t dropped[4] = {0, 0, 0, 0};
        int row(const keyframe *k) const { return k ? static_cast<int>(k - kfs.get()) : -1; }
    };

    void load(world &w, const snapshot &s)
    {
        w.F = s.F, w.L = s.L;
        w.kfs.reset(new keyframe[s.F > 0 ? s.F : 1]);
        w.lms.reset(new landmark[s.L > 0 ? s.L : 1]);
        keyframe *origin = nullptr;
        for (int f = 0; f < s.F; ++f)
        {
            keyframe &k = w.kfs[f];
            k.id_ = s.kf_id[f];
            if (s.has_origin && k.id_ == s.origin_id && !origin)
                origin = &k;
            k.undist_keypts_.resize(s.cap);
            k.stereo_x_right_.assign(s.cap, -1.0f);
            k.depths_.assign(s.cap, 0.0f);
            for (int i = 0; i < s.cap; ++i)
            {
                const size_t at = static_cast<size_t>(f) * s.kp_stride + i;
                if (s.undist)
                    k.undist_keypts_[i].octave = s.undist[at].octave;
                if (s.x_right)
                    k.stereo_x_right_[i] = s.x_right[at];
                if (s.depths)
                    k.depths_[i] = s.depths[at];
            }
            k.depth_thr_ = s.depth_thr ? s.depth_thr[f] : 0.0f;
            k.cannot_be_erased_ = s.kf_cannot_erase && s.kf_cannot_erase[f];
            k.will_be_erased_ = s.kf_erased && s.kf_erased[f];
        }
        for (int f = 0; f < s.F; ++f)
            w.kfs[f].origin_keyfrm_ = origin;
        for (int l = 0; l < s.L; ++l)
        {
            landmark &lm = w.lms[l];
            lm.will_be_erased_ = s.lm_erased && s.lm_erased[l];
            int lo = s.obs_offsets[l], hi = s.obs_offsets[l + 1];
            lo = lo < 0 ? 0 : (lo > s.T ? s.T : lo);
            hi = hi < lo ? lo : (hi > s.T ? s.T : hi);
            bool twice = false;
            for (int t = lo; t < hi; ++t)
            {
                const int kf = s.obs_kf[t], idx = s.obs_idx ? s.obs_idx[t] : 0;
                if (kf < 0 || kf >= s.F || idx < 0 || idx >= s.cap)
                {
                    ++w.dropped[1];
                    continue;
                }
                twice = twice || lm.observations_.count(&w.kfs[kf]);
                lm.add_observation(&w.kfs[kf], static_cast<unsigned>(idx));
            }
            w.dropped[2] += twice;
            if (s.lm_num_obs)
                lm.num_observations_ = s.lm_num_obs[l];
        }
        for (int f = 0; f < s.F; ++f)
        {
            int n = s.kf_counts ? s.kf_counts[f] : s.cap;
            n = n < 0 ? 0 : (n > s.cap ? s.cap : n);
            w.kfs[f].landmarks_.assign(n, nullptr);
            for (int i = 0; i < n; ++i)
            {
                const int v = s.kf_lm[static_cast<size_t>(f) * s.cap + i];
                if (0 <= v && v < s.L)
                    w.kfs[f].landmarks_[i] = &w.lms[v];
                else if (v != -1)
                    ++w.dropped[0];
            }
        }
    }

    struct graph_tables
    {
        int F, conn_cap, covis_cap;
        int32_t *kf_conn, *kf_conn_w, *kf_n_conn, *kf_covis, *kf_covis_w, *kf_n_covis, *kf_parent;
        uint8_t *kf_parent_unset;
    };

    // the tables into graph_node's private members; false when a table names a row outside [0, F) or a count outside its cap
    bool preset(world &w, const graph_tables &g)
    {
        for (int f = 0; f < g.F; ++f)
        {
            data::graph_node &n = *w.kfs[f].graph_node_;
            if (g.kf_n_conn[f] < 0 || g.kf_n_conn[f] > g.conn_cap || g.kf_n_covis[f] < 0 || g.kf_n_covis[f] > g.covis_cap)
                return false;
            for (int i = 0; i < g.kf_n_conn[f]; ++i)
            {
                const int j = g.kf_conn[static_cast<size_t>(f) * g.conn_cap + i];
                if (j < 0 || j >= g.F)
                    return false;
                n.connected_keyfrms_and_weights_[&w.kfs[j]] = static_cast<unsigned>(g.kf_conn_w[static_cast<size_t>(f) * g.conn_cap + i]);
            }
            for (int i = 0; i < g.kf_n_covis[f]; ++i)
            {
                const int j = g.kf_covis[static_cast<size_t>(f) * g.covis_cap + i];
                if (j < 0 || j >= g.F)
                    return false;
                n.ordered_covisibilities_.push_back(&w.kfs[j]);
                n.ordered_weights_.push_back(static_cast<unsigned>(g.kf_covis_w[static_cast<size_t>(f) * g.covis_cap + i]));
            }
            if (g.kf_parent)
            {
                if (g.kf_parent[f] >= g.F)
                    return false;
                n.spanning_parent_ = g.kf_parent[f] >= 0 ? &w.kfs[g.kf_parent[f]] : nullptr;
                n.spanning_parent_is_not_set_ = g.kf_parent_unset[f] != 0;
            }
        }
        return true;
    }

    // graph_node's members back into the tables, every row whole, -1 / 0 behind the last entry; false when a row outgrew its table
    bool readback(const world &w, const graph_tables &g)
    {
        bool fits = true;
        for (int f = 0; f < g.F; ++f)
        {
            const data::graph_node &n = *w.kfs[f].graph_node_;
            int i = 0;
            for (const auto &kw : n.connected_keyfrms_and_weights_)
            {
                if (i < g.conn_cap)
                {
                    g.kf_conn[static_cast<size_t>(f) * g.conn_cap + i] = w.row(kw.first);
                    g.kf_conn_w[static_cast<size_t>(f) * g.conn_cap + i] = static_cast<int32_t>(kw.second);
                }
                ++i;
            }
            g.kf_n_conn[f] = i;
            fits = fits && i <= g.conn_cap;
            for (; i < g.conn_cap; ++i)
                g.kf_conn[static_cast<size_t>(f) * g.conn_cap + i] = -1, g.kf_conn_w[static_cast<size_t>(f) * g.conn_cap + i] = 0;
            const int m = static_cast<int>(n.ordered_covisibilities_.size());
            fits = fits && m <= g.covis_cap && n.ordered_weights_.size() == n.ordered_covisibilities_.size();
            for (i = 0; i < g.covis_cap; ++i)
            {
                g.kf_covis[static_cast<size_t>(f) * g.covis_cap + i] = i < m ? w.row(n.ordered_covisibilities_[i]) : -1;
                g.kf_covis_w[static_cast<size_t>(f) * g.covis_cap + i] = i < m ? static_cast<int32_t>(n.ordered_weights_[i]) : 0;
            }
            g.kf_n_covis[f] = m;
            if (g.kf_parent)
            {
                g.kf_parent[f] = w.row(n.spanning_parent_);
                g.kf_parent_unset[f] = n.spanning_parent_is_not_set_ ? 1 : 0;
            }
        }
        return fits;
    }

    // update_connections() of key frame k.  The function returns nothing, so: a nullptr key put into the owner's connected map before the call
    // is still there iff the call returned at :123-126 without assigning (:180); nearest and max_weight are the head of the lists it assigned
    // (the assert of :187 holds them equal to the locals of :128-143).  Returns the status: 0 OK, 1 NO_SHARED.
    int update_one(world &w, int k, int32_t *nearest, int32_t *max_weight)
    {
        data::graph_node &n = *w.kfs[k].graph_node_;
        n.connected_keyfrms_and_weights_[nullptr] = 0;
        n.update_connections();
        if (n.connected_keyfrms_and_weights_.count(nullptr))
        {
            n.connected_keyfrms_and_weights_.erase(nullptr);
            *nearest = -1, *max_weight = 0;
            return 1;
        }
        *nearest = w.row(n.ordered_covisibilities_.front());
        *max_weight = static_cast<int32_t>(n.ordered_weights_.front());
        return 0;
    }

    graph_tables tables_of(const plp_covisibility_update_args *a)
    {
        return graph_tables{a->F, a->conn_cap, a->covis_cap, a->kf_conn, a->kf_conn_w, a->kf_n_conn, a->kf_covis, a->kf_covis_w, a->kf_n_covis,
                            a->kf_parent, a->kf_parent_unset};
    }

    graph_tables tables_of(const plp_covisibility_erase_args *a)
    {
        return graph_tables{a->F, a->conn_cap, a->covis_cap, a->kf_conn, a->kf_conn_w, a->kf_n_conn, a->kf_covis, a->kf_covis_w, a->kf_n_covis,
                            nullptr, nullptr};
    }

    // the in-table entries of problem g's list, cut to its first n entries; at[i] = the entry's place in the list
    std::vector<keyframe *> list_of(world &w, const plp_cull_keyframes_args *a, int g, int n, std::vector<int> *at = nullptr)
    {
        std::vector<keyframe *> lst;
        const int lo = a->covis_offsets[g];
        for (int j = 0; j < n; ++j)
        {
            const int c = a->covis[lo + j];
            if (c < 0 || c >= a->F)
                continue;
            lst.push_back(&w.kfs[c]);
            if (at)
                at->push_back(j);
        }
        return lst;
    }

    // set_origin_keyframe_id + remove_redundant_keyframes of problem g over a fresh copy of the map, its list cut to n entries
    unsigned run_problem(world &w, const plp_cull_keyframes_args *a, int g, int n, const module::local_map_cleaner &cleaner)
    {
        load(w, of(a));
        keyframe *cur = &w.kfs[a->cur_kf[g]];
        cur->graph_node_->ordered_covisibilities_ = list_of(w, a, g, n);
        return cleaner.remove_redundant_keyframes(cur);
    }
} // namespace

extern "C"
{
    // update_connections() of the owners, one after the other, over the state tables (in / out).  An owner outside [0, F) is status 2, a
    // repeated one 3, neither is run (what the C ABI adds to the text).  dropped[4]: see the head of this file.  0, or -1: a table does not fit.
    int ref3_covis_update(const plp_covisibility_update_args *a, int64_t *dropped)
    {
        world w;
        load(w, of(a));
        const graph_tables g = tables_of(a);
        if (!preset(w, g))
            return -1;
        std::set<int> done;
        for (int i = 0; i < a->G; ++i)
        {
            const int k = a->owners[i];
            int32_t nearest = -1, max_weight = 0;
            int status;
            if (k < 0 || k >= a->F)
                status = 2;
            else if (done.count(k))
                status = 3;
            else
                status = update_one(w, k, &nearest, &max_weight);
            done.insert(k);
            a->out_status[i] = static_cast<uint8_t>(status);
            if (a->out_nearest)
                a->out_nearest[i] = nearest;
            if (a->out_max_weight)
                a->out_max_weight[i] = max_weight;
        }
        if (dropped)
            std::memcpy(dropped, w.dropped, sizeof w.dropped);
        return readback(w, g) ? 0 : -1;
    }

    // erase_all_connections() of every key frame of the mask, in ascending row
    int ref3_covis_erase(const plp_covisibility_erase_args *a)
    {
        snapshot s;
        s.F = a->F;
        std::vector<uint32_t> ids(a->F > 0 ? a->F : 1);
        for (int f = 0; f < a->F; ++f)
            ids[f] = static_cast<uint32_t>(f) + 1;
        std::vector<int32_t> zero(2, 0);
        s.kf_id = ids.data(), s.obs_offsets = zero.data();
        world w;
        load(w, s);
        const graph_tables g = tables_of(a);
        if (!preset(w, g))
            return -1;
        for (int f = 0; f < a->F; ++f)
            if (a->erased[f])
                w.kfs[f].graph_node_->erase_all_connections();
        return readback(w, g) ? 0 : -1;
    }

    // Q queries over the state tables: kind 0 get_top_n_covisibilities(arg), 1 get_covisibilities_over_weight(arg), 2 get_weight(row arg; an
    // arg outside [0, F) is skipped: one value), 3 get_connected_keyframes() (a std::set: ascending row).  The answers are rows, written one
    // after another into out_values[out_cap]; out_offsets[Q + 1].  Returns the number of values, or -1.
    int ref3_covis_queries(const plp_covisibility_erase_args *a, int Q, const int32_t *rows, const int32_t *kind, const int32_t *arg, int32_t *out_offsets,
                           int32_t *out_values, int out_cap)
    {
        snapshot s;
        s.F = a->F;
        std::vector<uint32_t> ids(a->F > 0 ? a->F : 1);
        for (int f = 0; f < a->F; ++f)
            ids[f] = static_cast<uint32_t>(f) + 1;
        std::vector<int32_t> zero(2, 0);
        s.kf_id = ids.data(), s.obs_offsets = zero.data();
        world w;
        load(w, s);
        if (!preset(w, tables_of(a)))
            return -1;
        int n = 0;
        out_offsets[0] = 0;
        for (int q = 0; q < Q; ++q)
        {
            if (rows[q] < 0 || rows[q] >= a->F)
                return -1;
            const data::graph_node &node = *w.kfs[rows[q]].graph_node_;
            std::vector<int32_t> ans;
            if (kind[q] == 0)
                for (const auto k : node.get_top_n_covisibilities(static_cast<unsigned>(arg[q])))
                    ans.push_back(w.row(k));
            else if (kind[q] == 1)
                for (const auto k : node.get_covisibilities_over_weight(static_cast<unsigned>(arg[q])))
                    ans.push_back(w.row(k));
            else if (kind[q] == 2)
            {
                if (arg[q] < 0 || arg[q] >= a->F)
                    return -1;
                ans.push_back(static_cast<int32_t>(node.get_weight(&w.kfs[arg[q]])));
            }
            else
                for (const auto k : node.get_connected_keyframes())
                    ans.push_back(w.row(k));
            if (n + static_cast<int>(ans.size()) > out_cap)
                return -1;
            for (const auto v : ans)
                out_values[n++] = v;
            out_offsets[q + 1] = n;
        }
        return n;
    }

    // the public count_redundant_observations of every key frame of the snapshot: no stand-in behaviour involved
    int ref3_count_redundant(const plp_cull_keyframes_args *a, int32_t *out_num_valid, int32_t *out_num_redundant, int64_t *dropped)
    {
        world w;
        load(w, of(a));
        module::local_map_cleaner cleaner(a->is_monocular != 0);
        for (int f = 0; f < a->F; ++f)
        {
            unsigned nv = 0, nr = 0;
            cleaner.count_redundant_observations(&w.kfs[f], nv, nr);
            out_num_valid[f] = static_cast<int32_t>(nv), out_num_redundant[f] = static_cast<int32_t>(nr);
        }
        if (dropped)
            std::memcpy(dropped, w.dropped, sizeof w.dropped);
        return 0;
    }

    // set_origin_keyframe_id + remove_redundant_keyframes of every problem, each on a fresh copy of the map with the problem's list written
    // into the current key frame's ordered_covisibilities_.  out_num_removed[G] (-1: the current key frame is outside the table, nothing else
    // of the problem is written), out_kf_removed[G][F] and out_lm_erased[G][L]: the will_be_erased flags at the end.  Per entry of the lists,
    // derived from reference code alone by running every prefix: out_removed[Cv] (num_removed of the prefix that ends with the entry, minus
    // that of the one before; 255: the entry is outside the table and was not handed over), out_num_valid / out_num_redundant[Cv] (the
    // public count_redundant_observations of the entry in the state the prefix before it leaves) and out_flag[Cv] (the entry's will_be_erased
    // after its turn).  dropped[3] counts the entries and current key frames outside the table.
    int ref3_cull_keyframes(const plp_cull_keyframes_args *a, int32_t *out_num_removed, uint8_t *out_kf_removed, uint8_t *out_lm_erased,
                            uint8_t *out_removed, int32_t *out_num_valid, int32_t *out_num_redundant, uint8_t *out_flag, int64_t *dropped)
    {
        module::local_map_cleaner cleaner(a->is_monocular != 0);
        cleaner.set_origin_keyframe_id(a->origin_id);
        int64_t drop[4] = {0, 0, 0, 0};
        for (int g = 0; g < a->G; ++g)
        {
            const int lo = a->covis_offsets[g], n = a->covis_offsets[g + 1] - lo;
            if (a->cur_kf[g] < 0 || a->cur_kf[g] >= a->F)
            {
                out_num_removed[g] = -1;
                drop[3] += 1;
                continue;
            }
            unsigned before = 0;
            for (int j = 0; j < n; ++j)
            {
                const int c = a->covis[lo + j];
                if (c < 0 || c >= a->F)
                {
                    out_removed[lo + j] = 255;
                    drop[3] += 1;
                    continue;
                }
                world w;
                const unsigned upto = run_problem(w, a, g, j, cleaner); // the state at this entry's turn
                unsigned nv = 0, nr = 0;
                cleaner.count_redundant_observations(&w.kfs[c], nv, nr);
                world w2;
                const unsigned with = run_problem(w2, a, g, j + 1, cleaner);
                if (upto != before || with < upto || with > upto + 1)
                    return -2;
                out_removed[lo + j] = static_cast<uint8_t>(with - upto);
                out_num_valid[lo + j] = static_cast<int32_t>(nv), out_num_redundant[lo + j] = static_cast<int32_t>(nr);
                out_flag[lo + j] = w2.kfs[c].will_be_erased() ? 1 : 0;
                before = with;
            }
            world w;
            out_num_removed[g] = static_cast<int32_t>(run_problem(w, a, g, n, cleaner));
            for (int f = 0; f < a->F; ++f)
                out_kf_removed[static_cast<size_t>(g) * a->F + f] = w.kfs[f].will_be_erased() ? 1 : 0;
            for (int l = 0; l < a->L; ++l)
                out_lm_erased[static_cast<size_t>(g) * a->L + l] = w.lms[l].will_be_erased() ? 1 : 0;
            for (int k = 0; k < 3; ++k)
                drop[k] = w.dropped[k];
        }
        if (dropped)
            std::memcpy(dropped, drop, sizeof drop);
        return 0;
    }

    // add_fresh_landmark[_line] + remove_redundant_landmarks[_line] of every list.  Every ENTRY of a list is an object of its own with its
    // row's members (D20: entries are independent; the reference's buffer never holds a landmark twice), a row outside [0, L) is not handed
    // over (state 255, counted in dropped[3]).  Per entry: 0 HOLD (still in the buffer), 2 ERASE (will_be_erased rose in the call), 1 DROP.
    // The list afterwards is written into the list's own run of out_fresh.  is_monocular_ = (num_obs_thr[r] == 2).
    int ref3_cull_landmarks(const plp_cull_landmarks_args *a, int lines, int64_t *dropped)
    {
        int64_t drop[4] = {0, 0, 0, 0};
        for (int r = 0; r < a->R; ++r)
        {
            const int lo = a->fresh_offsets[r], n = a->fresh_offsets[r + 1] - lo;
            module::local_map_cleaner cleaner(a->num_obs_thr[r] == 2);
            cleaner._b_use_line_tracking = lines != 0;
            std::unique_ptr<landmark[]> lms(new landmark[n > 0 ? n : 1]);
            std::unique_ptr<data::Line[]> lns(new data::Line[n > 0 ? n : 1]);
            for (int j = 0; j < n; ++j)
            {
                const int v = a->fresh[lo + j];
                if (v < 0 || v >= a->L)
                {
                    a->out_state[lo + j] = 255;
                    drop[3] += 1;
                    continue;
                }
                if (lines)
                {
                    data::Line &ln = lns[j];
                    ln._will_be_erased = a->lm_erased && a->lm_erased[v];
                    ln._num_observed = a->num_observed[v], ln._num_observable = a->num_observable[v];
                    ln._first_keyfrm_id = a->first_kf_id[v], ln._num_observations = a->num_obs[v];
                    cleaner.add_fresh_landmark_line(&ln);
                }
                else
                {
                    landmark &lm = lms[j];
                    lm.will_be_erased_ = a->lm_erased && a->lm_erased[v];
                    lm.num_observed_ = a->num_observed[v], lm.num_observable_ = a->num_observable[v];
                    lm.first_keyfrm_id_ = a->first_kf_id[v], lm.num_observations_ = a->num_obs[v];
                    lm._mOwningPlane = (a->owning_plane && a->owning_plane[v]) ? reinterpret_cast<data::Plane *>(&lm) : nullptr;
                    cleaner.add_fresh_landmark(&lm);
                }
            }
            a->out_num_removed[r] = static_cast<int32_t>(lines ? cleaner.remove_redundant_landmarks_line(a->cur_kf_id[r])
                                                               : cleaner.remove_redundant_landmarks(a->cur_kf_id[r]));
            std::vector<uint8_t> held(n > 0 ? n : 1, 0);
            int m = 0;
            if (lines)
                for (const auto ln : cleaner._fresh_landmarks_line)
                    held[ln - lns.get()] = 1, a->out_fresh[lo + m++] = a->fresh[lo + (ln - lns.get())];
            else
                for (const auto lm : cleaner.fresh_landmarks_)
                    held[lm - lms.get()] = 1, a->out_fresh[lo + m++] = a->fresh[lo + (lm - lms.get())];
            a->out_num_fresh[r] = m;
            for (int j = 0; j < n; ++j)
            {
                const int v = a->fresh[lo + j];
                if (v < 0 || v >= a->L)
                    continue;
                const bool was = a->lm_erased && a->lm_erased[v];
                const bool is = lines ? lns[j].will_be_erased() : lms[j].will_be_erased();
                a->out_state[lo + j] = held[j] ? 0 : ((is && !was) ? 2 : 1);
            }
        }
        if (dropped)
            std::memcpy(dropped, drop, sizeof drop);
        return 0;
    }

    // The mapping loop's hand-over between the two modules on ONE set of objects: update_connections() of every key frame in ascending row
    // over an empty graph, then of `cur`; remove_redundant_keyframes(cur) with the list cur's own graph_node holds (prepare_for_erasing runs
    // the reference's erase_all_connections()); update_connections() of cur again.  out_list[F] / return value: cur's get_covisibilities()
    // before the cull.  The state tables of `u` receive the graph at the end; u's snapshot tables are not read (the cull's are the map).
    int ref3_chain(const plp_cull_keyframes_args *a, const plp_covisibility_update_args *u, int cur, int32_t *out_list, int32_t *out_num_removed,
                   uint8_t *out_kf_removed, uint8_t *out_lm_erased)
    {
        if (cur < 0 || cur >= a->F || u->F != a->F)
            return -1;
        world w;
        load(w, of(a));
        int32_t nearest, max_weight;
        for (int f = 0; f < a->F; ++f)
            update_one(w, f, &nearest, &max_weight);
        update_one(w, cur, &nearest, &max_weight);
        const auto lst = w.kfs[cur].graph_node_->get_covisibilities();
        for (size_t i = 0; i < lst.size(); ++i)
            out_list[i] = w.row(lst[i]);
        module::local_map_cleaner cleaner(a->is_monocular != 0);
        cleaner.set_origin_keyframe_id(a->origin_id);
        *out_num_removed = static_cast<int32_t>(cleaner.remove_redundant_keyframes(&w.kfs[cur]));
        for (int f = 0; f < a->F; ++f)
            out_kf_removed[f] = w.kfs[f].will_be_erased() ? 1 : 0;
        for (int l = 0; l < a->L; ++l)
            out_lm_erased[l] = w.lms[l].will_be_erased() ? 1 : 0;
        update_one(w, cur, &nearest, &max_weight);
        return readback(w, tables_of(u)) ? static_cast<int>(lst.size()) : -1;
    }
}
