// Stand-alone host program over csrc/local_ba.hpp for a sanitizer build (no GPU, no Python): a map of four key frames (two free, one fixed,
// one erased) and 30 landmarks through la_prepare, both rounds and la_finish with a team of one lane, on heap buffers of exact size (tables,
// outputs and the three state buffers), plus the 3 x 3 inverse on its edge arguments and a problem without a local key frame.
//
//   hipcc -std=c++17 -O1 -g -ffp-contract=off --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined tools/local_ba_host_check.hip -o local_ba_host_check
//   ./local_ba_host_check           # prints how far the free poses end from the truth and "ok"
#include <cmath>
#include <cstdio>
#include <memory>
#include <vector>

#include "../structure-plp-slam_amd/csrc/local_ba.hpp"

using namespace plp;

int main() {
    const int F = 4, L = 30, K = L;
    const PoseCam cam = pose_cam(458.654, 457.296, 367.215, 248.375, 50.4);
    std::vector<double> pose_gt(12 * F), pose(15 * F, 0.0), pos_gt(3 * L), pos_w(3 * L);
    for (int f = 0; f < F; ++f) {
        const double a = 0.05 * (f - 1.5), c = std::cos(a), s = std::sin(a);
        const double R[9] = {c, 0, s, 0, 1, 0, -s, 0, c}, t[3] = {-0.4 * (f - 1.5), 0.02 * f, 0.01 * f};
        for (int i = 0; i < 9; ++i) pose_gt[12 * f + i] = R[i];
        for (int i = 0; i < 3; ++i) pose_gt[12 * f + 9 + i] = t[i];
        for (int i = 0; i < 12; ++i) pose[15 * f + i] = pose_gt[12 * f + i];
        if (f < 2) { pose[15 * f + 9] += 0.03; pose[15 * f + 10] -= 0.02; }         // the free key frames start off the truth
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
            x_right[(size_t)f * K + l] = l % 2 ? (float)(kp.x - cam.fxb / z) : -1.0f;
            obs_kf[(size_t)l * F + f] = f; obs_idx[(size_t)l * F + f] = l;
        }
    undist[5].x += 45.0f;                                                            // one displaced observation of key frame 0
    obs_idx[7] = K + 3;                                                              // an index outside the key frame: not an edge
    const int T = L * F;
    std::vector<uint8_t> kf_erased = {0, 0, 0, 1}, kf_is_origin(F, 0), lm_erased(L, 0), kf_local = {1, 1, 0, 1, 0, 0, 0, 0};      // problem 1: nothing local
    lm_erased[4] = 1;
    const int G = 2;
    LaArgs A{};
    A.G = 1; A.F = F; A.L = L; A.T = T; A.kp_stride = K; A.pose_stride = 15; A.num_levels = 3; A.mono_setup = 0; A.it1 = 5; A.it2 = 10;
    A.cam = cam;
    A.delta_2d = (double)std::sqrt(kPoseChiSq2D); A.delta_3d = (double)std::sqrt(kPoseChiSq3D);
    for (int l = 0; l < 16; ++l) A.inv_sigma_sq[l] = l < 3 ? 1.0f / (1.0f + 0.44f * l) : 0.0f;
    A.pose = pose.data(); A.kf_erased = kf_erased.data(); A.kf_is_origin = kf_is_origin.data(); A.undist = undist.data(); A.x_right = x_right.data();
    A.counts = counts.data(); A.pos_w = pos_w.data(); A.lm_erased = lm_erased.data(); A.obs_offsets = off.data(); A.obs_kf = obs_kf.data(); A.obs_idx = obs_idx.data();
    std::vector<uint8_t> status(G, 9), kf_role((size_t)G * F, 9), lm_role((size_t)G * L, 9), outlier((size_t)G * T, 9);
    std::vector<double> out_pose((size_t)G * F * 15, -1.0), out_pos((size_t)G * L * 3, -1.0), rc(4 * G, -1.0);
    std::vector<int32_t> ri(8 * G, -1);
    std::unique_ptr<double[]> cd(new double[la_doubles(F, L, T)]);
    std::unique_ptr<int32_t[]> ci(new int32_t[la_ints(T)]);
    std::unique_ptr<uint8_t[]> cb(new uint8_t[la_bytes(F, L, T)]);
    A.ctx_d = cd.get(); A.ctx_i = ci.get(); A.ctx_b = cb.get();
    auto sh = std::make_unique<LaShared>();
    LaTeamHost par;
    for (int g = 0; g < G; ++g) {
        A.kf_local = kf_local.data() + (size_t)g * F;
        A.out_status = status.data() + g; A.out_kf_role = kf_role.data() + (size_t)g * F; A.out_lm_role = lm_role.data() + (size_t)g * L;
        A.out_pose = out_pose.data() + (size_t)g * F * 15; A.out_pos_w = out_pos.data() + (size_t)g * L * 3; A.out_outlier = outlier.data() + (size_t)g * T;
        A.out_round_info = ri.data() + 8 * g; A.out_round_chi2 = rc.data() + 4 * g;
        la_prepare(A, 0, *sh, par);
        la_solve(A, 0, *sh, par);
        la_finish(A, 0, par);
    }
    double err = 0.0;
    for (int f = 0; f < 2; ++f)
        for (int i = 0; i < 12; ++i) err = std::fmax(err, std::fabs(out_pose[15 * f + i] - pose_gt[12 * f + i]));
    // the 3 x 3 inverse on its edge arguments
    const double as[][6] = {{2, 0, 0, 3, 0, 4}, {1, 2, 3, 4, 6, 9}, {0, 0, 0, 0, 0, 0}, {NAN, 0, 0, 1, 0, 1}, {INFINITY, 0, 0, 1, 0, 1}, {1e300, 0, 0, 1e300, 0, 1e300}};
    std::unique_ptr<double[]> a6(new double[6]), o6(new double[6]);
    int oks = 0;
    for (const auto& row : as) {
        for (int i = 0; i < 6; ++i) a6[i] = row[i];
        oks = 2 * oks + (la_inv3(a6.get(), o6.get()) ? 1 : 0);
    }
    const bool good = status[0] == PLP_LOCAL_BA_OK && status[1] == PLP_LOCAL_BA_NO_EDGES && kf_role[0] == PLP_LOCAL_BA_KF_FREE && kf_role[2] == PLP_LOCAL_BA_KF_FIXED &&
                      kf_role[3] == PLP_LOCAL_BA_KF_NONE && lm_role[4] == 0 && outlier[5 * F] == 1 && outlier[7] == 9 && outlier[3] == 9 && err < 1e-3 && oks == 0b100000 &&
                      kf_role[F] == PLP_LOCAL_BA_KF_NONE && outlier[T] == 9;
    std::printf("pose error %.3g, rounds %d %d %d %d / %d %d %d %d, inverses %d: %s\n", err, ri[0], ri[1], ri[2], ri[3], ri[4], ri[5], ri[6], ri[7], oks, good ? "ok" : "FAILED");
    return good ? 0 : 1;
}
