// Stand-alone host program over csrc/transform_opt.hpp for a sanitizer build (no GPU, no Python): one synthetic pair of 40 matches through
// a linearisation, the 7 x 7 solve and five Levenberg-Marquardt iterations on heap buffers of exact size, plus exp, Sim3(update) and the
// Cholesky on their edge arguments.
//
//   hipcc -std=c++17 -O1 -g -ffp-contract=off --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined tools/transform_opt_host_check.hip -o transform_opt_host_check
//   ./transform_opt_host_check           # prints the scale it converged to and "ok"
#include <cmath>
#include <cstdio>
#include <memory>
#include <vector>

#include "../structure-plp-slam_amd/csrc/transform_opt.hpp"

using namespace plp;

int main() {
    const int n = 40;
    const PoseCam cam = pose_cam(458.654, 457.296, 367.215, 248.375, 0.0);
    // truth: Sim3_12 = (I, (0.1, -0.05, 0.02), 1.1); both key frames at the world's origin
    const double st = 1.1, tt[3] = {0.1, -0.05, 0.02};
    std::vector<double> pc1(3 * n), pc2(3 * n), obs1(2 * n), obs2(2 * n);
    for (int k = 0; k < n; ++k) {
        const double z = 3.0 + 0.15 * k, x = (k % 7 - 3) * 0.3 * z / 3.0, y = (k % 5 - 2) * 0.25 * z / 3.0;
        pc1[3 * k] = x; pc1[3 * k + 1] = y; pc1[3 * k + 2] = z;
        for (int i = 0; i < 3; ++i) pc2[3 * k + i] = (pc1[3 * k + i] - tt[i]) / st;
        obs1[2 * k] = (float)(cam.fx * x / z + cam.cx); obs1[2 * k + 1] = (float)(cam.fy * y / z + cam.cy);
        obs2[2 * k] = (float)(cam.fx * pc2[3 * k] / pc2[3 * k + 2] + cam.cx); obs2[2 * k + 1] = (float)(cam.fy * pc2[3 * k + 1] / pc2[3 * k + 2] + cam.cy);
    }
    auto W = std::make_unique<TfWork>();
    const double rot[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, t0[3] = {0.12, -0.03, 0.0};
    tf_est_from_input(rot, t0, 1.07f, W->est);
    W->ni = 2.0;
    const double delta = (double)std::sqrt(10.0f);
    auto pass = [&](bool lin, double* sums) {
        std::unique_ptr<double[]> T(new double[kTfTerms]);
        for (int t = 0; t < kTfTerms; ++t) sums[t] = 0.0;
        for (int k = 0; k < n; ++k)
            for (int dir = 0; dir < 2; ++dir) {
                const double* p = (dir ? pc1.data() : pc2.data()) + 3 * k;     // the landmark in the other key frame's camera
                const double* o = (dir ? obs2.data() : obs1.data()) + 2 * k;
                const double* sims = dir ? W->invs : W->sims;
                if (lin) {
                    tf_edge_terms(sims, cam, p[0], p[1], p[2], o[0], o[1], 1.0, delta, T.get(), 1);
                    for (int t = 0; t < kTfTerms; ++t) sums[t] = sums[t] + T[t];
                } else {
                    double e0, e1, rho0, rho1;
                    pose_huber(tf_edge_error(sims + 8 * 14, cam, p[0], p[1], p[2], o[0], o[1], 1.0, e0, e1), delta, rho0, rho1);
                    sums[35] = sums[35] + rho0;
                }
            }
    };
    std::unique_ptr<double[]> sums(new double[kTfTerms]);
    for (int it = 0; it < 5; ++it) {
        for (int i = 0; i < kTfSims; ++i) { tf_perturb(W->est, i, false, W->sims + 8 * i); tf_inverse(W->sims + 8 * i, W->invs + 8 * i); }
        pass(true, W->sum);
        lev_begin<kTfDim>(*W, it);
        do {
            tf_lm_solve(*W);
            tf_lm_update(*W, false);
            pass(false, sums.get());
            lev_decide_vertex<kTfDim, 8>(*W, sums[35]);
        } while (W->go_on);
        if (lev_end(*W)) break;
    }
    // the edge arguments of the pieces
    const double xs[] = {0.0, 700.0, -700.0, 700.5, -1e300, 1e-300, NAN, INFINITY, -INFINITY};
    double acc = 0.0;
    for (double x : xs) { const double v = pose_exp(x); acc += v == v ? 0.0 : 1.0; }
    std::unique_ptr<double[]> u(new double[7]), out(new double[8]), inv(new double[8]), w13(new double[13]);
    const double us[][7] = {{0, 0, 0, 0, 0, 0, 0}, {1e-9, 0, 0, 0, 0, 0, 0}, {0, 0, 0, 0, 0, 0, -1e-9}, {0.3, -0.2, 0.1, 1, 2, 3, 0.2}, {1e-7, 0, 0, 1, 1, 1, 0.5},
                            {2e6, 0, 0, 0, 0, 0, 0}, {0, 0, 0, 0, 0, 0, 800.0}, {NAN, 0, 0, 0, 0, 0, 0}};
    for (const auto& row : us) {
        for (int i = 0; i < 7; ++i) u[i] = row[i];
        tf_oplus(u.get(), false, W->est, out.get());
        tf_oplus(u.get(), true, W->est, out.get());
        tf_inverse(out.get(), inv.get());
    }
    const double pose2[15] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0.5, 0.25, 1.0, 0, 0, 0};
    tf_world_to_1(W->est, pose2, w13.get());
    std::unique_ptr<double[]> H(new double[28]), b(new double[7]), Lf(new double[49]), y(new double[7]), x(new double[7]);
    for (int i = 0; i < 28; ++i) H[i] = 0.0;
    for (int i = 0; i < 7; ++i) b[i] = 1.0;
    const bool ok0 = lev_chol<kTfDim>(H.get(), b.get(), 0.0, Lf.get(), y.get(), x.get());      // no information: fails
    const bool ok1 = lev_chol<kTfDim>(H.get(), b.get(), 0.5, Lf.get(), y.get(), x.get());      // lambda alone: x = b / lambda
    const bool good = !ok0 && ok1 && std::fabs(x[6] - 2.0) < 1e-12 && acc == 5.0 && std::fabs(W->est[7] - st) < 1e-5 && std::fabs(W->est[4] - tt[0]) < 1e-5;
    std::printf("scale %.9f trans %.6f %.6f %.6f rejected %d, solves %d %d x6 %g, NaN of exp %g: %s\n", W->est[7], W->est[4], W->est[5], W->est[6], W->rejected,
                (int)ok0, (int)ok1, x[6], acc, good ? "ok" : "FAILED");
    return good ? 0 : 1;
}
