// Stand-alone host program over csrc/plane_fit.hpp for a sanitizer build (no GPU, no Python): the fit, the draws, the replay of the loop and
// refine_points on heap buffers of exact size -- a noisy plane with outliers and holes through the whole CREATE and UPDATE procedure as the
// host build runs it (a team of one), a fit of one point, of 64 and 65 equal points, a void sample, a NaN position, and the move of points
// on both sides of a plane.
//
//   hipcc -std=c++17 -O1 -g -ffp-contract=off --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined tools/plane_host_check.hip -o plane_host_check
//   ./plane_host_check           # prints one line per scene and "ok"
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <memory>
#include <vector>

#include "../structure-plp-slam_amd/csrc/plane_fit.hpp"

using namespace plp;

namespace {
struct Lcg {                                          // a small generator of the program's own
    uint64_t s;
    double next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (double)(s >> 11) / 9007199254740992.0; }
    double sym() { return 2.0 * next() - 1.0; }
};

// the plane z = 0.25 x - 0.5 y + 3 with noise, every seventh point far off, every eleventh erased, every thirteenth unowned
void make_scene(int n, Lcg& g, double* pos, uint8_t* flags) {
    for (int i = 0; i < n; ++i) {
        const double x = 2.0 * g.sym(), y = 2.0 * g.sym();
        double z = 0.25 * x - 0.5 * y + 3.0 + 0.002 * g.sym();
        if (i % 7 == 3) z += 0.5 + g.next();
        pos[3 * i] = x; pos[3 * i + 1] = y; pos[3 * i + 2] = z;
        flags[i] = PLP_PLANE_LM_OWNED;
        if (i % 11 == 5) { flags[i] |= PLP_PLANE_LM_ERASED; pos[3 * i + 1] = NAN; }
        if (i % 13 == 6) flags[i] &= (uint8_t)~PLP_PLANE_LM_OWNED;
    }
}

// one problem as plane_context.hip's host build runs it; returns the status
int run_problem(int mode, int n, int iters, double best_error_in, double* out_eq, int* out_num) {
    Lcg g{(uint64_t)(1000 * mode + n)};
    std::unique_ptr<double[]> pos(new double[3 * (size_t)n]);
    std::unique_ptr<uint8_t[]> flags(new uint8_t[(size_t)n]);
    make_scene(n, g, pos.get(), flags.get());
    PlaneArgs A{};
    A.mode = mode; A.P = 1; A.n_cap = n; A.iters = iters; A.points_per_ransac = 18; A.min_points_before_ransac = 12; A.inliers_ratio_thr = 0.7; A.seed = 42;
    std::vector<int> elig, live;
    for (int s = 0; s < n; ++s) {
        if (plane_eligible(mode, flags[s])) elig.push_back(s);
        if (plane_live(flags[s])) live.push_back(s);
    }
    int fl = 0;
    const int early = plane_early_status(A, n, (int)elig.size(), fl);
    if (early != PLP_PLANE_OK) return early;
    const int m = plane_sample_size(mode, n, A.points_per_ransac);
    const double thr = 0.02, error_thresh = 0.002;
    std::unique_ptr<double[]> eq_s(new double[4 * (size_t)iters]), eq_r(new double[4 * (size_t)iters]), res(new double[(size_t)iters]), err(new double[(size_t)iters]);
    std::unique_ptr<uint8_t[]> tried(new uint8_t[(size_t)iters]);
    auto T = std::make_unique<PlaneHostTeam>();
    std::vector<int> list;
    for (int it = 0; it < iters; ++it) {
        int sweeps = 0;
        plane_fit(*T, [&](int k, double x[3]) {
            const int rank = it == 1 ? (int)elig.size() : ransac_draw_one(A.seed, 0, it, k, (int)elig.size());   // iteration 1: a void sample
            if ((unsigned)rank >= (unsigned)elig.size()) return false;
            for (int r = 0; r < 3; ++r) x[r] = pos[3 * (size_t)elig[rank] + r];
            return true;
        }, m, &eq_s[4 * (size_t)it], res[it], sweeps);
        const double abs_n = plane_abs_n(&eq_s[4 * (size_t)it]);
        list.clear();
        for (int s : live)
            if (plane_distance(&eq_s[4 * (size_t)it], abs_n, &pos[3 * (size_t)s]) < thr) list.push_back(s);
        tried[it] = plane_refit_gate(A, n, (int)list.size()) ? 1 : 0;
        err[it] = kPlaneMax;
        for (int i = 0; i < 4; ++i) eq_r[4 * (size_t)it + i] = 0.0;
        if (tried[it])
            plane_fit(*T, [&](int k, double x[3]) {
                for (int r = 0; r < 3; ++r) x[r] = pos[3 * (size_t)list[k] + r];
                return true;
            }, (int)list.size(), &eq_r[4 * (size_t)it], err[it], sweeps);
    }
    const PlaneReplay R = plane_replay(mode, iters, best_error_in, error_thresh, [&](int i) { return res[i]; }, [&](int i) { return tried[i] != 0; },
                                       [&](int i) { return err[i]; });
    int status = plane_late_status(mode, R, error_thresh, fl);
    const double* eq = R.last_refit ? &eq_r[4 * (size_t)R.last_iter] : &eq_s[4 * (size_t)R.last_iter];
    for (int i = 0; i < 4; ++i) out_eq[i] = eq[i];
    *out_num = 0;
    if (status == PLP_PLANE_OK) {
        const double* eq_b = &eq_s[4 * (size_t)R.best_iter];
        for (int s : live)
            if (plane_distance(eq_b, plane_abs_n(eq_b), &pos[3 * (size_t)s]) < thr && plane_distance(eq, plane_abs_n(eq), &pos[3 * (size_t)s]) < thr) ++*out_num;
        if (mode == PLP_PLANE_UPDATE && *out_num < A.points_per_ransac) status = PLP_PLANE_TOO_FEW_LEFT;
    }
    return status;
}

bool fit_equal_points(int m) {
    std::unique_ptr<double[]> pos(new double[3]{1.5, -2.0, 0.25});
    auto T = std::make_unique<PlaneHostTeam>();
    double eq[4], res;
    int sweeps;
    plane_fit(*T, [&](int, double x[3]) { x[0] = pos[0]; x[1] = pos[1]; x[2] = pos[2]; return true; }, m, eq, res, sweeps);
    const double n2 = eq[0] * eq[0] + eq[1] * eq[1] + eq[2] * eq[2];
    std::printf("fit of %d equal points: normal^2 %.17g, residual %.3g\n", m, n2, res);
    return std::fabs(n2 - 1.0) < 1e-15 && res < 1e-15;
}

bool refine_scene() {
    const int M = 9, NP = 2;
    std::unique_ptr<double[]> pos(new double[3 * M]), eq(new double[4 * NP]{0.0, 0.0, 2.0, -4.0, 1.0, 0.0, 0.0, 0.0}), thr(new double[1]{0.02});
    std::unique_ptr<int32_t[]> owner(new int32_t[M]{0, 0, 0, 0, 1, -1, 2, 0, 0});
    std::unique_ptr<uint8_t[]> flags(new uint8_t[M]), active(new uint8_t[NP]{1, 0}), changed(new uint8_t[M]);
    const double z[M] = {2.01, 1.99, 2.0, 2.5, 0.0, 2.01, 2.01, 2.01, 2.01};
    for (int i = 0; i < M; ++i) { pos[3 * i] = 0.5 * i; pos[3 * i + 1] = -1.0; pos[3 * i + 2] = z[i]; flags[i] = PLP_PLANE_LM_OWNED; }
    flags[7] |= PLP_PLANE_LM_ERASED; flags[8] = 0;
    PlaneRefineArgs A{};
    A.M = M; A.NP = NP; A.pos_w = pos.get(); A.lm_plane = owner.get(); A.flags = flags.get(); A.equation = eq.get(); A.active = active.get();
    A.dist_thresh = thr.get(); A.out_changed = changed.get();
    for (int i = 0; i < M; ++i) plane_refine_landmark(A, i);
    // above the plane, near or far (dist_old is not held against the threshold): moves onto it
    bool good = changed[0] == 1 && std::fabs(pos[2] - 2.0) < 1e-15 && changed[3] == 1 && std::fabs(pos[11] - 2.0) < 1e-15;
    for (int i = 1; i < M; ++i)                                     // below (moves away), on it, inactive, no owner, out of range, erased, unowned
        if (i != 3) good = good && changed[i] == 0 && pos[3 * i + 2] == z[i];
    std::printf("refine_points: %s\n", good ? "ok" : "FAILED");
    return good;
}
}  // namespace

int main() {
    bool good = true;
    double eq[4];
    int num;
    const int st_c = run_problem(PLP_PLANE_CREATE, 300, 50, 0.0, eq, &num);
    std::printf("CREATE n = 300: status %d, %d members, normal (%.6f, %.6f, %.6f) d %.6f\n", st_c, num, eq[0], eq[1], eq[2], eq[3]);
    good = good && st_c == PLP_PLANE_OK && num > 200 && std::fabs(eq[0] / eq[2] + 0.25) < 1e-3 && std::fabs(eq[1] / eq[2] - 0.5) < 1e-3;
    const int st_u = run_problem(PLP_PLANE_UPDATE, 257, 12, kPlaneMax, eq, &num);
    std::printf("UPDATE n = 257: status %d, %d members\n", st_u, num);
    good = good && (st_u == PLP_PLANE_OK || st_u == PLP_PLANE_NOT_FOUND || st_u == PLP_PLANE_ERROR_ABOVE_THRESHOLD || st_u == PLP_PLANE_TOO_FEW_LEFT);
    good = good && run_problem(PLP_PLANE_CREATE, 11, 4, 0.0, eq, &num) == PLP_PLANE_TOO_FEW_POINTS;
    good = good && run_problem(PLP_PLANE_UPDATE, 17, 4, 1.0, eq, &num) == PLP_PLANE_TOO_FEW_POINTS;
    good = good && fit_equal_points(1) && fit_equal_points(64) && fit_equal_points(65);
    {   // the draws stay in range at both ends; the sample size of UPDATE
        int lo = 1 << 30, hi = -1;
        for (int k = 0; k < 20000; ++k) { const int r = ransac_draw_one(7, 65534, 1023, k, 8192); lo = r < lo ? r : lo; hi = r > hi ? r : hi; }
        good = good && lo >= 0 && hi < 8192 && ransac_draw_one(1, 0, 0, 0, 1) == 0;
        good = good && plane_sample_size(PLP_PLANE_UPDATE, 8192, 18) == 6554 && plane_sample_size(PLP_PLANE_UPDATE, 5, 18) == 4 && plane_sample_size(PLP_PLANE_UPDATE, 0, 18) == 0;
        std::printf("draws in [%d, %d]\n", lo, hi);
    }
    {   // a NaN position: the fit ends, with a NaN residual that is below nothing
        std::unique_ptr<double[]> pos(new double[12]{0, 0, 0, 1, 0, 0, 0, 1, 0, NAN, 1, 1});
        auto T = std::make_unique<PlaneHostTeam>();
        double res;
        int sweeps;
        plane_fit(*T, [&](int k, double x[3]) { for (int r = 0; r < 3; ++r) x[r] = pos[3 * k + r]; return true; }, 4, eq, res, sweeps);
        good = good && res != res && sweeps < kJacobiSweepLimit;
        std::printf("NaN position: residual %g after %d sweeps\n", res, sweeps);
    }
    good = good && refine_scene();
    std::printf("%s\n", good ? "ok" : "FAILED");
    return good ? 0 : 1;
}
