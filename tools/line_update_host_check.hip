// Stand-alone host program over csrc/line_update.hpp for a sanitizer build (no GPU, no Python): 9 key frames of 37 key-line slots and 600 lines with
// ragged observation lists, on heap buffers of exact size, through line_trim_item in both modes, line_correct_item and line_propagate_item.  Among the
// rows: reference key frames outside the table (-1, F, far beyond) and erased ones, lists that do not hold the reference key frame, a feature index of
// -1, at counts[ref], at cap and far beyond, a NaN and an infinite pose entry, exactly horizontal and vertical reprojections (l1 == 0, l2 == 0) from an
// identity pose, Sim3 rows with an infinite scale, key-frame statuses of every kind, the end points written over the old ones.
//
//   hipcc -std=c++17 -O1 -g --offload-arch=gfx950 -ffp-contract=off -Xarch_host -fsanitize=address,undefined tools/line_update_host_check.hip -o line_update_host_check
//   ./line_update_host_check         # prints the census of every status and "ok"
#include <cmath>
#include <cstdio>
#include <memory>
#include <vector>

#include "../structure-plp-slam_amd/csrc/line_update.hpp"

using namespace plp;

static uint32_t rnd_state = 2929u;
static int rnd(int n) { rnd_state = rnd_state * 1664525u + 1013904223u; return (int)((rnd_state >> 8) % (uint32_t)n); }
static double unit() { return rnd(20001) / 10000.0 - 1.0; }

template <class T> static std::unique_ptr<T[]> exact(const std::vector<T>& v) {     // a heap block of exactly the vector's size
    std::unique_ptr<T[]> p(new T[v.size() ? v.size() : 1]);
    for (size_t i = 0; i < v.size(); ++i) p[i] = v[i];
    return p;
}

static void rot(double ax, double ay, double az, double* R) {
    const double cx = cos(ax), sx = sin(ax), cy = cos(ay), sy = sin(ay), cz = cos(az), sz = sin(az);
    const double r[9] = {cz * cy, cz * sy * sx - sz * cx, cz * sy * cx + sz * sx, sz * cy, sz * sy * sx + cz * cx, sz * sy * cx - cz * sx, -sy, cy * sx, cy * cx};
    for (int i = 0; i < 9; ++i) R[i] = r[i];
}

int main() {
    const int F = 9, L = 600, cap = 37, stride = 13;
    const double fx = 520.0, fy = 515.0, cx = 320.5, cy = 240.25;
    std::vector<double> pose((size_t)F * stride, 1e30), after((size_t)F * 15), before((size_t)F * 12), sim_cw((size_t)F * 8), sim_wc((size_t)F * 8);
    std::vector<uint8_t> kf_erased(F, 0), kf_status(F);
    std::vector<int32_t> counts(F);
    std::vector<float> median(F);
    std::vector<plp_keyline> kl((size_t)F * cap);
    for (int f = 0; f < F; ++f) {
        double R[9], t[3] = {0.5 * unit(), 0.5 * unit(), 0.5 * unit()};
        rot(f ? 0.1 * unit() : 0.0, f ? 0.1 * unit() : 0.0, f ? 0.1 * unit() : 0.0, R);
        if (!f) t[0] = t[1] = t[2] = 0.0;                       // key frame 0: the identity pose
        for (int i = 0; i < 9; ++i) pose[(size_t)f * stride + i] = before[(size_t)f * 12 + i] = R[i];
        for (int i = 0; i < 3; ++i) pose[(size_t)f * stride + 9 + i] = before[(size_t)f * 12 + 9 + i] = t[i];
        double R2[9];
        rot(0.1 * unit(), 0.1 * unit(), 0.1 * unit(), R2);
        for (int i = 0; i < 9; ++i) after[(size_t)f * 15 + i] = R2[i];
        for (int i = 0; i < 3; ++i) after[(size_t)f * 15 + 9 + i] = t[i] + 0.1 * unit();
        for (int i = 0; i < 3; ++i)
            after[(size_t)f * 15 + 12 + i] = -(R2[i] * after[(size_t)f * 15 + 9] + R2[3 + i] * after[(size_t)f * 15 + 10] + R2[6 + i] * after[(size_t)f * 15 + 11]);
        for (int s = 0; s < 2; ++s) {
            double* q = (s ? sim_wc : sim_cw).data() + (size_t)8 * f;
            double n = 0.0;
            for (int i = 0; i < 4; ++i) { q[i] = i == 3 ? 3.0 + unit() : unit(); n += q[i] * q[i]; }
            for (int i = 0; i < 4; ++i) q[i] /= sqrt(n);
            for (int i = 0; i < 3; ++i) q[4 + i] = unit();
            q[7] = 1.0 + 0.05 * unit();
        }
        counts[f] = f == 4 ? cap + 5 : f == 5 ? -3 : cap - rnd(6);   // above the row width, negative, ragged
        median[f] = f == 6 ? 0.0f : 5.0f;
        kf_status[f] = (uint8_t)(f % 4);
        for (int j = 0; j < cap; ++j) {
            plp_keyline& k = kl[(size_t)f * cap + j];
            k = plp_keyline{};
            k.startPointX = (float)(320.0 + 200.0 * unit()); k.startPointY = (float)(240.0 + 150.0 * unit());
            k.endPointX = (float)(320.0 + 200.0 * unit()); k.endPointY = (float)(240.0 + 150.0 * unit());
        }
    }
    kf_erased[7] = 1;
    pose[(size_t)8 * stride + 10] = NAN;
    pose[(size_t)3 * stride + 2] = INFINITY;
    sim_cw[(size_t)8 * 2 + 7] = INFINITY;
    std::vector<double> pk((size_t)L * 6), old((size_t)L * 6), pk_after((size_t)L * 6);
    std::vector<int32_t> ref(L), corr(L), off(L + 1, 0), obs_kf, obs_idx;
    std::vector<uint8_t> skip(L), opt(L);
    for (int l = 0; l < L; ++l) {
        double sp[3] = {1.5 * unit(), unit(), 5.5 + 2.5 * unit()}, d[3] = {unit(), unit(), 0.5 * unit()};
        if (l % 50 == 7) { d[1] = d[2] = 0.0; }                  // parallel to x: horizontal from the identity pose
        if (l % 50 == 8) { d[0] = d[2] = 0.0; }                  // parallel to y: vertical
        pk[(size_t)6 * l] = sp[1] * d[2] - sp[2] * d[1]; pk[(size_t)6 * l + 1] = sp[2] * d[0] - sp[0] * d[2]; pk[(size_t)6 * l + 2] = sp[0] * d[1] - sp[1] * d[0];
        for (int i = 0; i < 3; ++i) {
            pk[(size_t)6 * l + 3 + i] = d[i];
            old[(size_t)6 * l + i] = sp[i]; old[(size_t)6 * l + 3 + i] = sp[i] + d[i];
        }
        for (int i = 0; i < 6; ++i) pk_after[(size_t)6 * l + i] = pk[(size_t)6 * l + i] * 1.01;
        const int sel = rnd(40);
        ref[l] = (l % 50 == 7 || l % 50 == 8) ? 0 : sel == 0 ? -1 : sel == 1 ? F : sel == 2 ? 1 << 30 : sel == 3 ? 7 : rnd(F);
        corr[l] = rnd(30) == 0 ? F + rnd(3) : rnd(30) == 0 ? -1 - rnd(3) : rnd(4) ? ref[l] : rnd(F);
        skip[l] = rnd(15) == 0;
        opt[l] = rnd(3) == 0;
        const int n = rnd(8) == 0 ? 0 : 1 + rnd(F);
        bool has = false;
        for (int o = 0; o < n; ++o) {
            int k = rnd(10) == 0 ? -1 - rnd(3) : rnd(10) == 0 ? F + rnd(3) : rnd(F);
            if (o == n - 1 && !has && rnd(6)) k = ref[l];
            has = has || k == ref[l];
            const int c = (unsigned)k < (unsigned)F ? counts[k] : cap;
            const int sidx = rnd(12);
            obs_kf.push_back(k);
            obs_idx.push_back(sidx == 0 ? -1 : sidx == 1 ? c : sidx == 2 ? cap : sidx == 3 ? 1 << 29 : sidx == 4 ? -7 : rnd(cap));
        }
        off[l + 1] = (int32_t)obs_kf.size();
    }
    auto h_pose = exact(pose); auto h_after = exact(after); auto h_before = exact(before); auto h_cw = exact(sim_cw); auto h_wc = exact(sim_wc);
    auto h_er = exact(kf_erased); auto h_st = exact(kf_status); auto h_cnt = exact(counts); auto h_med = exact(median); auto h_kl = exact(kl);
    auto h_pk = exact(pk); auto h_old = exact(old); auto h_pka = exact(pk_after); auto h_ref = exact(ref); auto h_corr = exact(corr); auto h_off = exact(off);
    auto h_okf = exact(obs_kf); auto h_oidx = exact(obs_idx); auto h_skip = exact(skip); auto h_opt = exact(opt);
    std::unique_ptr<double[]> o_pos(new double[(size_t)L * 6]), o_pk(new double[(size_t)L * 6]);
    std::unique_ptr<uint8_t[]> o_st(new uint8_t[L]), o_erase(new uint8_t[L]);

    bool good = true;
    for (int mode = 0; mode < 2; ++mode)
        for (int with_counts = 0; with_counts < 2; ++with_counts) {
            LineTrimArgs A{};
            A.L = L; A.F = F; A.cap = cap; A.pose_stride = stride; A.mode = mode; A.fx = fx; A.fy = fy; A.cx = cx; A.cy = cy; A.max_change = 0.1;
            A.pluecker = h_pk.get(); A.ref_kf = h_ref.get(); A.skip = with_counts ? h_skip.get() : nullptr; A.obs_offsets = h_off.get(); A.obs_kf = h_okf.get();
            A.obs_idx = h_oidx.get(); A.pose = h_pose.get(); A.kf_erased = h_er.get(); A.kl = h_kl.get(); A.counts = with_counts ? h_cnt.get() : nullptr;
            for (size_t i = 0; i < (size_t)L * 6; ++i) o_pos[i] = old[i];
            A.pos_w_old = mode ? o_pos.get() : nullptr; A.median = mode ? h_med.get() : nullptr;   // the end points written over the old ones
            A.out_pos_w = o_pos.get(); A.out_status = o_st.get(); A.out_erase = o_erase.get();
            int census[6] = {0, 0, 0, 0, 0, 0}, erased = 0, nan_ok = 0;
            for (int l = 0; l < L; ++l) {
                line_trim_item(A, l);
                good = good && o_st[l] < 6 && o_erase[l] == (o_st[l] == PLP_TRIM_NOT_OBSERVED || o_st[l] == PLP_TRIM_REJECTED);
                ++census[o_st[l] < 6 ? o_st[l] : 0];
                erased += o_erase[l];
                if (o_st[l] == PLP_TRIM_OK && std::isnan(o_pos[(size_t)6 * l])) ++nan_ok;
                if (o_st[l] != PLP_TRIM_OK) for (int i = 0; i < 6; ++i) good = good && o_pos[(size_t)6 * l + i] == old[(size_t)6 * l + i];
            }
            printf("trim mode %d counts %d: ok %d skipped %d no_ref %d not_observed %d index_range %d rejected %d, erase %d, ok with NaN %d\n", mode, with_counts,
                   census[0], census[1], census[2], census[3], census[4], census[5], erased, nan_ok);
            for (int s = with_counts ? 0 : 2; s < 6; ++s) good = good && census[s] > 0;
            good = good && (mode == PLP_TRIM_DEPTH_POSITIVE ? nan_ok == 0 : nan_ok > 0);      // a NaN compares false (D25)
        }
    {
        LineCorrectArgs A{};
        A.L = L; A.F = F; A.pluecker = h_pk.get(); A.lm_erased = h_skip.get(); A.ref_kf = h_ref.get(); A.corr_kf = h_corr.get(); A.kf_erased = h_er.get();
        A.sim3_cw = h_cw.get(); A.corrected_wc = h_wc.get(); A.out_pluecker = o_pk.get(); A.out_status = o_st.get();
        int census[4] = {0, 0, 0, 0}, nan_rows = 0;
        for (int l = 0; l < L; ++l) {
            line_correct_item(A, l);
            good = good && o_st[l] < 4;
            ++census[o_st[l] < 4 ? o_st[l] : 0];
            if (o_st[l] == PLP_CORRECT_LINE_OK && std::isnan(o_pk[(size_t)6 * l + 5])) ++nan_rows;   // 0 * inf of the lower left block
        }
        printf("correct: ok %d erased %d no_ref %d no_vertex %d, NaN rows %d\n", census[0], census[1], census[2], census[3], nan_rows);
        for (int s = 0; s < 4; ++s) good = good && census[s] > 0;
        good = good && nan_rows > 0;
    }
    {
        LinePropagateArgs A{};
        A.L = L; A.F = F; A.pose_after = h_after.get(); A.pose_before = h_before.get(); A.kf_status = h_st.get(); A.pluecker = h_pk.get(); A.lm_erased = h_skip.get();
        A.ref_kf = h_ref.get(); A.line_optimized = h_opt.get(); A.pluecker_after = h_pka.get(); A.out_pluecker = o_pk.get(); A.out_status = o_st.get();
        int census[4] = {0, 0, 0, 0};
        for (int l = 0; l < L; ++l) {
            line_propagate_item(A, l);
            good = good && o_st[l] < 4;
            ++census[o_st[l] < 4 ? o_st[l] : 0];
        }
        printf("propagate: no_ref %d optimized %d moved %d erased %d\n", census[0], census[1], census[2], census[3]);
        for (int s = 0; s < 4; ++s) good = good && census[s] > 0;
    }
    printf(good ? "ok\n" : "FAILED\n");
    return good ? 0 : 1;
}
