// Stand-alone host program over plp_model_local_ba_lines_host (csrc/local_ba_lines.hpp with a team of one lane) for a sanitizer build (no GPU is
// used, no Python): one small built-in scene -- four key frames on a line (two local, two that become constant vertices, one of them through a line
// only), nine landmarks and six lines seen from the exact projections, perturbed starts, one displaced key point and one displaced key-line end
// point -- on heap arrays of exact size, both rounds.
//
//   cd structure-plp-slam_amd/csrc && hipcc -std=c++17 -O1 -g -ffp-contract=off --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined \
//       ../../tools/local_ba_lines_host_check.hip local_ba_lines_context.hip local_ba_lines_kernels.hip plp_core.hip -o local_ba_lines_host_check
//   ./local_ba_lines_host_check      # prints the rounds' records and "ok"
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../include/plp_front.h"

int main() {
    const int F = 4, L = 9, LL = 6, K = 12, KL = 8;
    const double fx = 458.654, fy = 457.296, cx = 367.215, cy = 248.375, fxb = 50.4;
    plp_local_ba_lines_args a{};
    plp_local_ba_args& p = a.points;
    p.camera.model = PLP_CAMERA_PERSPECTIVE; p.camera.cols = 752; p.camera.rows = 480;
    p.camera.fx = fx; p.camera.fy = fy; p.camera.cx = cx; p.camera.cy = cy; p.camera.focal_x_baseline = fxb;
    p.setup_type = 2; p.num_first_iter = 5; p.num_second_iter = 10; p.G = 1; p.F = F; p.L = L; p.kp_stride = K; p.pose_stride = 12;
    std::vector<float> sigma = {1.0f, 0.69f, 0.48f}, sigma_lsd = {1.0f, 0.25f};
    p.inv_level_sigma_sq = sigma.data(); p.num_levels = 3; a.inv_level_sigma_sq_lsd = sigma_lsd.data(); a.num_levels_lsd = 2;
    // key frame f looks along z from (0.5 f, 0, 0); the start of the two local ones is moved
    std::vector<double> pose_gt(12 * F, 0.0), pose(12 * F, 0.0);
    for (int f = 0; f < F; ++f) {
        for (int i = 0; i < 3; ++i) pose_gt[12 * f + 4 * i] = 1.0;
        pose_gt[12 * f + 9] = -0.5 * f;
        for (int i = 0; i < 12; ++i) pose[12 * f + i] = pose_gt[12 * f + i];
    }
    pose[9] += 0.02; pose[10] -= 0.01; pose[12 + 11] += 0.015;
    std::vector<uint8_t> kf_local = {1, 1, 0, 0};
    std::vector<plp_keypoint> undist((size_t)F * K);
    std::vector<float> x_right((size_t)F * K, -1.0f);
    std::vector<int32_t> counts(F, 0), kl_counts(F, 0);
    std::vector<plp_keyline> keylines((size_t)F * KL);
    for (auto& k : undist) { k = plp_keypoint{}; k.octave = 99; }
    for (auto& k : keylines) { k = plp_keyline{}; k.octave = 99; }
    auto project = [&](int f, const double* P, double& u, double& v, double& z) {
        const double x = P[0] + pose_gt[12 * f + 9], y = P[1];
        z = P[2];
        u = fx * x / z + cx; v = fy * y / z + cy;
    };
    // landmarks: seen by the key frames 0, 1, 2 (never by 3)
    std::vector<double> pos_w(3 * L);
    std::vector<int32_t> obs_offsets(1, 0), obs_kf, obs_idx;
    for (int l = 0; l < L; ++l) {
        const double P[3] = {-1.0 + 0.4 * l, 0.5 - 0.13 * l, 5.0 + 0.3 * (l % 4)};
        for (int i = 0; i < 3; ++i) pos_w[3 * l + i] = P[i] + 0.01 * ((l + i) % 3 - 1);
        for (int f = 0; f < 3; ++f) {
            if ((l + f) % 4 == 3) continue;
            double u, v, z;
            project(f, P, u, v, z);
            const int i = counts[f]++;
            plp_keypoint& k = undist[(size_t)f * K + i];
            k.x = (float)u; k.y = (float)v; k.octave = (l + f) % 3;
            if (l % 2) x_right[(size_t)f * K + i] = (float)(u - fxb / z);
            obs_kf.push_back(f); obs_idx.push_back(i);
        }
        obs_offsets.push_back((int32_t)obs_kf.size());
    }
    undist[0].x += 40.0f;                                     // a displaced key point (three views: the landmark follows it)
    // lines: seen by every key frame, so that key frame 3 is a vertex through the lines alone
    std::vector<double> pluecker(6 * LL);
    std::vector<int32_t> obs_offsets_lines(1, 0), obs_kf_lines, obs_idx_lines;
    for (int l = 0; l < LL; ++l) {
        const double S[3] = {-1.2 + 0.5 * l, -0.6 + 0.1 * l, 5.5 + 0.2 * l}, E[3] = {S[0] + 0.6, S[1] + 0.5 - 0.15 * l, S[2] + 0.4};
        double d[3] = {E[0] - S[0], E[1] - S[1], E[2] - S[2]};
        const double n = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
        for (double& v : d) v /= n;
        const double Sp[3] = {S[0] + 0.01, S[1] - 0.01, S[2] + 0.02};
        pluecker[6 * l + 0] = Sp[1] * d[2] - Sp[2] * d[1]; pluecker[6 * l + 1] = Sp[2] * d[0] - Sp[0] * d[2]; pluecker[6 * l + 2] = Sp[0] * d[1] - Sp[1] * d[0];
        for (int i = 0; i < 3; ++i) pluecker[6 * l + 3 + i] = d[i];
        for (int f = 0; f < F; ++f) {
            double us, vs, ue, ve, z;
            project(f, S, us, vs, z);
            project(f, E, ue, ve, z);
            const int i = kl_counts[f]++;
            plp_keyline& k = keylines[(size_t)f * KL + i];
            k.startPointX = (float)us; k.startPointY = (float)vs; k.endPointX = (float)ue; k.endPointY = (float)ve; k.octave = (l + f) % 2;
            obs_kf_lines.push_back(f); obs_idx_lines.push_back(i);
        }
        obs_offsets_lines.push_back((int32_t)obs_kf_lines.size());
    }
    keylines[(size_t)2 * KL + 1].startPointY += 45.0f;        // a displaced end point
    const int T = (int)obs_kf.size(), TL = (int)obs_kf_lines.size();
    p.T = T; a.LL = LL; a.TL = TL; a.kl_stride = KL;
    p.pose = pose.data(); p.undist = undist.data(); p.x_right = x_right.data(); p.counts = counts.data(); p.pos_w = pos_w.data();
    p.obs_offsets = obs_offsets.data(); p.obs_kf = obs_kf.data(); p.obs_idx = obs_idx.data(); p.kf_local = kf_local.data();
    a.keylines = keylines.data(); a.kl_counts = kl_counts.data(); a.pluecker = pluecker.data(); a.obs_offsets_lines = obs_offsets_lines.data();
    a.obs_kf_lines = obs_kf_lines.data(); a.obs_idx_lines = obs_idx_lines.data();
    std::vector<uint8_t> status(1, 77), kf_role(F, 77), lm_role(L, 77), outlier(T, 77), line_role(LL, 77), outlier_lines(TL, 77);
    std::vector<double> out_pose(15 * F, -7.5), out_pos(3 * L, -7.5), out_pk(6 * LL, -7.5), chi2(4, -7.5);
    std::vector<int32_t> info(8, -7);
    p.out_status = status.data(); p.out_kf_role = kf_role.data(); p.out_lm_role = lm_role.data(); p.out_pose = out_pose.data(); p.out_pos_w = out_pos.data();
    p.out_outlier = outlier.data(); p.out_round_info = info.data(); p.out_round_chi2 = chi2.data();
    a.out_line_role = line_role.data(); a.out_pluecker = out_pk.data(); a.out_outlier_lines = outlier_lines.data();
    const int32_t r = plp_model_local_ba_lines_host(&a);
    bool good = r == 1 && status[0] == PLP_LOCAL_BA_OK;
    good = good && kf_role[0] == PLP_LOCAL_BA_KF_FREE && kf_role[1] == PLP_LOCAL_BA_KF_FREE && kf_role[2] == PLP_LOCAL_BA_KF_FIXED && kf_role[3] == PLP_LOCAL_BA_KF_FIXED;
    for (int l = 0; l < LL; ++l) {
        good = good && line_role[l] == 1;
        for (int i = 0; i < 6; ++i) good = good && std::isfinite(out_pk[6 * l + i]);
    }
    for (int f = 0; f < 2; ++f)
        for (int i = 0; i < 15; ++i) good = good && std::isfinite(out_pose[15 * f + i]);
    for (int i = 0; i < 15; ++i) good = good && out_pose[15 * 2 + i] == -7.5;     // a constant vertex's row keeps the caller's value
    int bad_points = 0, bad_lines = 0;
    for (uint8_t v : outlier) bad_points += v == 1;
    for (uint8_t v : outlier_lines) bad_lines += v == 1;
    good = good && bad_lines >= 1 && info[0] >= 2 && info[4] >= 2 && info[2] >= 1 && chi2[2] <= chi2[0];
    std::printf("status %d, rounds (iterations, rejected, to level 1, end) (%d %d %d %d) (%d %d %d %d), chi2 %.6g -> %.6g, outliers %d points %d line edges: %s\n", status[0],
                info[0], info[1], info[2], info[3], info[4], info[5], info[6], info[7], chi2[0], chi2[2], bad_points, bad_lines, good ? "ok" : "FAILED");
    return good ? 0 : 1;
}
