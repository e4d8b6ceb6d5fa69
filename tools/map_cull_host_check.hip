// Stand-alone host program over csrc/map_cull.hpp for a sanitizer build (no GPU, no Python): a generated map of 70 key frames of up to 257 key
// points and 900 landmarks with erased rows, rows outside their tables, counts below and above the row width, stereo weights and depth gates (a
// NaN among them), six problems (an empty list, a current key frame outside the table, entries outside it) through cull_replay and cull_masks,
// and four fresh lists through cull_states, with a team of one lane, on heap buffers of exact size.
//
//   hipcc -std=c++17 -O1 -g --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined tools/map_cull_host_check.hip -o map_cull_host_check
//   ./map_cull_host_check            # prints every problem's counts and "ok"
#include <cmath>
#include <cstdio>
#include <memory>
#include <vector>

#include "../structure-plp-slam_amd/csrc/map_cull.hpp"

using namespace plp;

static uint32_t rnd_state = 2222u;
static int rnd(int n) { rnd_state = rnd_state * 1664525u + 1013904223u; return (int)((rnd_state >> 8) % (uint32_t)n); }

template <class T> static std::unique_ptr<T[]> exact(const std::vector<T>& v) {     // a heap block of exactly the vector's size
    std::unique_ptr<T[]> p(new T[v.size() ? v.size() : 1]);
    for (size_t i = 0; i < v.size(); ++i) p[i] = v[i];
    return p;
}

int main() {
    const int F = 70, L = 900, cap = 257, stride = 260;
    std::vector<int32_t> kf_lm((size_t)F * cap, -1), kf_counts(F), off(L + 1, 0), obs_kf, obs_idx;
    std::vector<plp_keypoint> undist((size_t)F * stride);
    std::vector<float> x_right((size_t)F * stride), depths((size_t)F * stride), depth_thr(F, 40.0f);
    std::vector<uint32_t> kf_id(F);
    std::vector<uint8_t> cannot(F), lm_erased(L);
    std::vector<int> used(F, 0);
    for (int f = 0; f < F; ++f) {
        kf_id[f] = f == 5 ? 3u : 10u + f;
        cannot[f] = f % 8 == 0;
        for (int i = 0; i < stride; ++i) {
            undist[(size_t)f * stride + i].octave = f % 4 == 0 ? 9 : rnd(3);
            x_right[(size_t)f * stride + i] = rnd(3) ? (float)rnd(600) : -1.0f;
            depths[(size_t)f * stride + i] = rnd(40) == 0 ? -1.0f : rnd(40) == 0 ? 50.0f : rnd(40) == 0 ? NAN : (float)(1 + rnd(30));
        }
    }
    for (int l = 0; l < L; ++l) {
        lm_erased[l] = rnd(20) == 0;
        const int n = l % 100 == 7 ? F : l % 25 == 3 ? rnd(4) : 4 + rnd(5);       // most lists long enough for a coarse key frame to be redundant
        for (int i = 0; i < n; ++i) {
            const int kf = n == F ? i : (l / 13 + rnd(12)) % F;
            if (used[kf] >= cap) continue;
            bool twice = false;
            for (size_t t = (size_t)off[l]; t < obs_kf.size(); ++t) twice = twice || obs_kf[t] == kf;
            if (twice) continue;
            kf_lm[(size_t)kf * cap + used[kf]] = l;
            obs_kf.push_back(rnd(60) == 0 ? F + 1 : kf); obs_idx.push_back(rnd(60) == 0 ? cap : used[kf]);
            ++used[kf];
        }
        off[l + 1] = (int32_t)obs_kf.size();
    }
    for (int f = 0; f < F; ++f) {
        kf_counts[f] = f == 3 ? cap + 4 : f == 4 ? -1 : used[f] + rnd(3);
        if (used[f] < cap) kf_lm[(size_t)f * cap + used[f]] = rnd(2) ? L + 5 : -9;        // a row outside the table behind the last landmark
    }
    std::vector<int32_t> cur = {60, 61, F, 62, -1, 63}, covis_off = {0}, covis;
    for (int g = 0; g < 6; ++g) {
        const int n = g == 1 ? 0 : g == 3 ? 1 : 66;
        for (int i = 0; i < n; ++i) covis.push_back(rnd(25) == 0 ? F + 2 : rnd(25) == 0 ? -1 : (i * 11 + g) % F);
        covis_off.push_back((int32_t)covis.size());
    }
    const int G = 6, Cv = (int)covis.size(), words = (F + 31) / 32;
    auto p_kl = exact(kf_lm); auto p_kc = exact(kf_counts); auto p_un = exact(undist); auto p_xr = exact(x_right); auto p_dp = exact(depths);
    auto p_dt = exact(depth_thr); auto p_id = exact(kf_id); auto p_ce = exact(cannot); auto p_of = exact(off); auto p_ok = exact(obs_kf);
    auto p_oi = exact(obs_idx); auto p_le = exact(lm_erased); auto p_cu = exact(cur); auto p_co = exact(covis_off); auto p_cv = exact(covis);
    auto n_rem = exact(std::vector<int32_t>(G, -9)); auto dec = exact(std::vector<uint8_t>(Cv, 99)); auto nv = exact(std::vector<int32_t>(Cv, -9));
    auto nr = exact(std::vector<int32_t>(Cv, -9)); auto kf_rem = exact(std::vector<uint8_t>((size_t)G * F, 99));
    auto lm_dead = exact(std::vector<uint8_t>((size_t)G * L, 99));
    CullArgs A{};
    A.F = F; A.L = L; A.T = (int)obs_kf.size(); A.cap = cap; A.kp_stride = stride; A.G = G; A.Cv = Cv; A.mono = 0; A.origin_id = 3u;
    A.kf_lm = p_kl.get(); A.kf_counts = p_kc.get(); A.undist = p_un.get(); A.x_right = p_xr.get(); A.depths = p_dp.get(); A.depth_thr = p_dt.get();
    A.kf_id = p_id.get(); A.kf_cannot_erase = p_ce.get(); A.obs_offsets = p_of.get(); A.obs_kf = p_ok.get(); A.obs_idx = p_oi.get();
    A.lm_erased = p_le.get(); A.cur_kf = p_cu.get(); A.covis_offsets = p_co.get(); A.covis = p_cv.get();
    A.out_num_removed = n_rem.get(); A.out_decision = dec.get(); A.out_num_valid = nv.get(); A.out_num_redundant = nr.get();
    A.out_kf_removed = kf_rem.get(); A.out_lm_erased = lm_dead.get(); A.words = words;
    std::unique_ptr<uint32_t[]> rem(new uint32_t[(size_t)G * words]);
    std::unique_ptr<int32_t[]> cnt(new int32_t[(size_t)Cv * 2]);
    A.rem = rem.get(); A.cnt = cnt.get();
    auto sh = std::make_unique<CullShared>();
    LmTeamHost par;
    bool good = true;
    int seen = 0;
    for (int j = 0; j < Cv; ++j) cull_count_entry(A, j, *sh, par);
    for (int g = 0; g < G; ++g) {
        cull_replay(A, g, *sh, par);
        for (int i = 0; i < cull_mask_rows(A); ++i) cull_masks(A, g, i, sh->rem);
        int removed = 0, dead = 0;
        for (int j = covis_off[g]; j < covis_off[g + 1]; ++j) {
            seen |= 1 << dec[j];
            const bool counted = dec[j] == PLP_CULL_KF_KEPT || dec[j] == PLP_CULL_KF_REMOVED || dec[j] == PLP_CULL_KF_REMOVED_HELD;
            good = good && dec[j] <= PLP_CULL_KF_ABSENT && counted == (nv[j] != -9) && (!counted || (0 <= nr[j] && nr[j] <= nv[j] && nv[j] <= cap));
            removed += dec[j] == PLP_CULL_KF_REMOVED || dec[j] == PLP_CULL_KF_REMOVED_HELD;
        }
        for (int l = 0; l < L; ++l) { good = good && lm_dead[(size_t)g * L + l] <= 1 && lm_dead[(size_t)g * L + l] >= lm_erased[l]; dead += lm_dead[(size_t)g * L + l]; }
        for (int f = 0; f < F; ++f) good = good && kf_rem[(size_t)g * F + f] == (uint8_t)cull_bit(rem.get() + (size_t)g * words, f);
        good = good && n_rem[g] == removed;
        std::printf("problem %d: %d entries, removed %d, landmarks dead %d\n", g, covis_off[g + 1] - covis_off[g], n_rem[g], dead);
    }
    good = good && (seen & 0x3f) == 0x3f;                             // every decision code
    // the replay alone gives what the replay over the snapshot counts gave
    auto dec2 = exact(std::vector<uint8_t>(Cv, 99)); auto nv2 = exact(std::vector<int32_t>(Cv, -9)); auto nr2 = exact(std::vector<int32_t>(Cv, -9));
    A.cnt = nullptr; A.out_decision = dec2.get(); A.out_num_valid = nv2.get(); A.out_num_redundant = nr2.get();
    for (int g = 0; g < G; ++g) cull_replay(A, g, *sh, par);
    for (int j = 0; j < Cv; ++j) good = good && dec2[j] == dec[j] && nv2[j] == nv[j] && nr2[j] == nr[j];

    const int R = 4, LN = 500;
    std::vector<uint32_t> observed(LN), observable(LN), first(LN), num_obs(LN), cur_id = {50u, 50u, 51u, 0u}, thr = {2u, 3u, 3u, 2u};
    std::vector<uint8_t> erased(LN), plane(LN);
    for (int l = 0; l < LN; ++l) {
        observed[l] = rnd(12); observable[l] = rnd(12); first[l] = l == 0 ? 0xFFFFFFFEu : 44u + rnd(9); num_obs[l] = rnd(7);
        erased[l] = rnd(12) == 0; plane[l] = rnd(5) == 0;
    }
    std::vector<int32_t> fresh, fresh_off = {0};
    for (int r = 0; r < R; ++r) {
        const int n = r == 0 ? 0 : r == 1 ? 1 : r == 2 ? 300 : 257;
        for (int i = 0; i < n; ++i) fresh.push_back(rnd(50) == 0 ? LN : rnd(50) == 0 ? -1 : rnd(LN));
        fresh_off.push_back((int32_t)fresh.size());
    }
    const int N = (int)fresh.size();
    auto q_fo = exact(fresh_off); auto q_fr = exact(fresh); auto q_er = exact(erased); auto q_od = exact(observed); auto q_ob = exact(observable);
    auto q_fi = exact(first); auto q_no = exact(num_obs); auto q_pl = exact(plane); auto q_cu = exact(cur_id); auto q_th = exact(thr);
    auto state = exact(std::vector<uint8_t>(N, 99)); auto removed = exact(std::vector<int32_t>(R, -9)); auto kept = exact(std::vector<int32_t>(R, -9));
    auto list = exact(std::vector<int32_t>(N, -9));
    CullLmArgs B{};
    B.R = R; B.N = N; B.L = LN; B.fresh_offsets = q_fo.get(); B.fresh = q_fr.get(); B.lm_erased = q_er.get(); B.num_observed = q_od.get();
    B.num_observable = q_ob.get(); B.first_kf_id = q_fi.get(); B.num_obs = q_no.get(); B.owning_plane = q_pl.get(); B.cur_kf_id = q_cu.get();
    B.num_obs_thr = q_th.get(); B.out_state = state.get(); B.out_num_removed = removed.get(); B.out_num_fresh = kept.get(); B.out_fresh = list.get();
    CullSharedLm shl{};
    for (int r = 0; r < R; ++r) {
        cull_states(B, r, shl, par);
        int hold = 0, erase = 0;
        for (int e = fresh_off[r]; e < fresh_off[r + 1]; ++e) {
            good = good && state[e] <= PLP_CULL_ERASE;
            if (state[e] == PLP_CULL_HOLD) good = good && list[fresh_off[r] + hold++] == fresh[e];
            erase += state[e] == PLP_CULL_ERASE;
        }
        good = good && kept[r] == hold && removed[r] == erase && (fresh_off[r] + hold == fresh_off[r + 1] || list[fresh_off[r] + hold] == -9);
        std::printf("list %d: %d entries, %d held, %d erased\n", r, fresh_off[r + 1] - fresh_off[r], kept[r], removed[r]);
    }
    std::printf("decisions seen 0x%x: %s\n", seen, good ? "ok" : "FAILED");
    return good ? 0 : 1;
}
