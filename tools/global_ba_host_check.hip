// Stand-alone host program over csrc/global_ba.hpp for a sanitizer build (no GPU, no Python): a map of six key frames (the origin, four free, one
// erased) and 40 landmarks through gb_run_host on heap buffers of exact size, with and without the Huber kernel and with `stop` set; the dense
// Cholesky and both substitutions at n = 0, 1 and 70 against a residual; the map update over a tree with a cycle, a broken link and an erased key frame.
//
//   hipcc -std=c++17 -O1 -g -ffp-contract=off --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined tools/global_ba_host_check.hip -o global_ba_host_check
//   ./global_ba_host_check           # prints how far the free poses end from the truth, the residual and "ok"
#include <cmath>
#include <cstdio>
#include <vector>

#include "../structure-plp-slam_amd/csrc/global_ba.hpp"

using namespace plp;

int main() {
    const int F = 6, L = 40, K = L;
    const PoseCam cam = pose_cam(458.654, 457.296, 367.215, 248.375, 50.4);
    std::vector<double> pose_gt(12 * F), pose(15 * F, 0.0), pos_gt(3 * L), pos_w(3 * L);
    for (int f = 0; f < F; ++f) {
        const double a = 0.05 * (f - 2.5), c = std::cos(a), s = std::sin(a);
        const double R[9] = {c, 0, s, 0, 1, 0, -s, 0, c}, t[3] = {-0.4 * (f - 2.5), 0.02 * f, 0.01 * f};
        for (int i = 0; i < 9; ++i) pose_gt[12 * f + i] = R[i];
        for (int i = 0; i < 3; ++i) pose_gt[12 * f + 9 + i] = t[i];
        for (int i = 0; i < 12; ++i) pose[15 * f + i] = pose_gt[12 * f + i];
        if (f > 0) { pose[15 * f + 9] += 0.03; pose[15 * f + 10] -= 0.02; }          // every key frame but the origin starts off the truth
    }
    for (int l = 0; l < L; ++l) {
        pos_gt[3 * l] = (l % 6 - 2.5) * 0.7; pos_gt[3 * l + 1] = (l % 5 - 2) * 0.5; pos_gt[3 * l + 2] = 5.0 + 0.1 * l;
        for (int i = 0; i < 3; ++i) pos_w[3 * l + i] = pos_gt[3 * l + i] + 0.01 * ((l + i) % 3 - 1);
    }
    std::vector<plp_keypoint> undist((size_t)F * K);
    std::vector<float> x_right((size_t)F * K);
    std::vector<int32_t> counts(F, K), off(L + 1), obs_kf((size_t)L * F), obs_idx((size_t)L * F);
    for (int l = 0; l <= L; ++l) off[l] = l * F;
    for (int l = 0; l < L; ++l)
        for (int f = 0; f < F; ++f) {
            const double* P = &pose_gt[12 * f];
            const double x = P[0] * pos_gt[3 * l] + P[1] * pos_gt[3 * l + 1] + P[2] * pos_gt[3 * l + 2] + P[9];
            const double y = P[3] * pos_gt[3 * l] + P[4] * pos_gt[3 * l + 1] + P[5] * pos_gt[3 * l + 2] + P[10];
            const double z = P[6] * pos_gt[3 * l] + P[7] * pos_gt[3 * l + 1] + P[8] * pos_gt[3 * l + 2] + P[11];
            plp_keypoint& kp = undist[(size_t)f * K + l];
            kp = plp_keypoint{};
            kp.x = (float)(cam.fx * x / z + cam.cx); kp.y = (float)(cam.fy * y / z + cam.cy); kp.octave = l % 3;
            x_right[(size_t)f * K + l] = (float)(kp.x - cam.fxb / z);
            obs_kf[(size_t)l * F + f] = f; obs_idx[(size_t)l * F + f] = l;
        }
    obs_idx[7] = K + 3;                                                              // an index outside the key frame: not an edge
    obs_kf[9] = F + 2;                                                               // a key frame outside the table
    const int T = L * F;
    std::vector<uint8_t> kf_erased = {0, 0, 0, 0, 0, 1}, kf_is_origin = {1, 0, 0, 0, 0, 0}, lm_erased(L, 0);
    lm_erased[4] = 1;
    GbArgs A{};
    A.F = F; A.L = L; A.T = T; A.kp_stride = K; A.pose_stride = 15; A.num_levels = 3;
    A.cam = cam;
    A.delta = (double)std::sqrt(kPoseChiSq3D);
    for (int l = 0; l < 16; ++l) A.inv_sigma_sq[l] = l < 3 ? 1.0f / (1.0f + 0.44f * l) : 0.0f;
    A.pose = pose.data(); A.kf_erased = kf_erased.data(); A.kf_is_origin = kf_is_origin.data(); A.undist = undist.data(); A.x_right = x_right.data();
    A.counts = counts.data(); A.pos_w = pos_w.data(); A.lm_erased = lm_erased.data(); A.obs_offsets = off.data(); A.obs_kf = obs_kf.data(); A.obs_idx = obs_idx.data();
    std::vector<uint8_t> status(1), kf_opt(F), lm_opt(L);
    std::vector<double> out_pose(15 * F, -7.0), out_pos(3 * L, -7.0), chi2(3);
    std::vector<int32_t> info(4);
    A.out_status = status.data(); A.out_kf_optimized = kf_opt.data(); A.out_lm_optimized = lm_opt.data(); A.out_pose = out_pose.data(); A.out_pos_w = out_pos.data();
    A.out_info = info.data(); A.out_chi2 = chi2.data();
    double worst = 0.0;
    for (int robust = 0; robust < 2; ++robust) {
        GbArgs B = A;
        B.robust = robust;
        gb_run_host(B, 10, nullptr);
        if (status[0] != PLP_GLOBAL_BA_OK || info[0] < 1 || !(chi2[1] <= chi2[0])) { std::printf("run %d: status %d, %d iterations, chi2 %g -> %g\n", robust, status[0], info[0], chi2[0], chi2[1]); return 1; }
        for (int f = 0; f < F - 1; ++f)
            for (int i = 0; i < 12; ++i) worst = std::fmax(worst, std::fabs(out_pose[15 * f + i] - pose_gt[12 * f + i]));
        if (kf_opt[F - 1] != 0 || out_pose[15 * (F - 1)] != -7.0 || lm_opt[4] != 0 || out_pos[12] != -7.0) { std::printf("an erased row was written\n"); return 1; }
    }
    std::printf("free poses end %.3g from the truth\n", worst);
    if (!(worst < 1e-3)) return 1;
    volatile int32_t stop = 1;
    { GbArgs B = A; status[0] = 99; gb_run_host(B, 10, &stop); if (status[0] != PLP_GLOBAL_BA_STOPPED) return 1; }

    // the dense solve
    for (int n : {0, 1, 70}) {
        std::vector<double> M((size_t)n * n), S((size_t)n * n), b(n), x(n);
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < n; ++j) M[(size_t)i * n + j] = std::sin(1.0 + i * 0.7 + j * 1.3) + (i == j ? 3.0 : 0.0);
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < n; ++j) {
                double s = 0.0;
                for (int k = 0; k < n; ++k) s += M[(size_t)i * n + k] * M[(size_t)j * n + k];
                S[(size_t)i * n + j] = s;
            }
        const std::vector<double> A0 = S;
        for (int i = 0; i < n; ++i) x[i] = b[i] = std::cos(0.3 * i);
        if (!gb_chol_host(S.data(), n)) return 1;
        gb_subst_host(S.data(), n, x.data());
        double res = 0.0;
        for (int i = 0; i < n; ++i) {
            double s = -b[i];
            for (int j = 0; j < n; ++j) s += A0[(size_t)i * n + j] * x[j];
            res = std::fmax(res, std::fabs(s));
        }
        std::printf("n = %d: residual %.3g\n", n, res);
        if (!(res < 1e-9)) return 1;
    }

    // the map update: 0 the origin, 1 - 2 a chain below it, 3 unoptimised below 2, 4 <-> 5 a cycle, 6 a broken link, 7 erased, 8 below the erased one
    const int PF = 9, PL = 12;
    std::vector<int32_t> parent = {-1, 0, 1, 2, 5, 4, 40, 1, 7}, ref(PL);
    std::vector<uint8_t> optimized = {1, 1, 1, 0, 0, 0, 0, 1, 0}, p_erased = {0, 0, 0, 0, 0, 0, 0, 1, 0}, origin = {1, 0, 0, 0, 0, 0, 0, 0, 0}, l_opt(PL), l_erased(PL, 0);
    std::vector<double> p_pose(15 * PF, 0.0), p_after(15 * PF, 0.0), p_pos(3 * PL), p_posa(3 * PL);
    for (int f = 0; f < PF; ++f)
        for (int i = 0; i < 12; ++i) { p_pose[15 * f + i] = pose_gt[12 * (f % F) + i]; p_after[15 * f + i] = pose_gt[12 * ((f + 1) % F) + i]; }
    for (int l = 0; l < PL; ++l) {
        ref[l] = l - 1; l_opt[l] = l % 3 == 0;
        for (int i = 0; i < 3; ++i) { p_pos[3 * l + i] = pos_gt[3 * l + i]; p_posa[3 * l + i] = pos_gt[3 * l + i] + 0.1; }
    }
    l_erased[2] = 1;
    std::vector<double> o_pose(15 * PF, -7.0), o_before(12 * PF, -7.0), o_pos(3 * PL, -7.0);
    std::vector<uint8_t> o_kf(PF, 99), o_lm(PL, 99);
    LpArgs Q{};
    Q.F = PF; Q.L = PL; Q.pose_stride = 15;
    Q.pose = p_pose.data(); Q.kf_erased = p_erased.data(); Q.kf_is_origin = origin.data(); Q.kf_parent = parent.data(); Q.kf_optimized = optimized.data(); Q.pose_after = p_after.data();
    Q.pos_w = p_pos.data(); Q.lm_erased = l_erased.data(); Q.ref_kf = ref.data(); Q.lm_optimized = l_opt.data(); Q.pos_after = p_posa.data();
    Q.out_pose = o_pose.data(); Q.out_pose_before = o_before.data(); Q.out_kf_status = o_kf.data(); Q.out_pos_w = o_pos.data(); Q.out_lm_status = o_lm.data();
    for (int f = 0; f < PF; ++f) lp_kf_out(Q, f);
    for (int l = 0; l < PL; ++l) lp_lm_item(Q, l);
    const uint8_t want[PF] = {PLP_LOOP_BA_KF_OPTIMIZED, PLP_LOOP_BA_KF_OPTIMIZED, PLP_LOOP_BA_KF_OPTIMIZED, PLP_LOOP_BA_KF_PROPAGATED, PLP_LOOP_BA_KF_NOT_REACHED,
                              PLP_LOOP_BA_KF_NOT_REACHED, PLP_LOOP_BA_KF_NOT_REACHED, PLP_LOOP_BA_KF_ERASED, PLP_LOOP_BA_KF_NOT_REACHED};
    for (int f = 0; f < PF; ++f)
        if (o_kf[f] != want[f]) { std::printf("key frame %d: status %d, expected %d\n", f, o_kf[f], want[f]); return 1; }
    std::printf("ok\n");
    return 0;
}
