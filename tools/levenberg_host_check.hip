// Stand-alone host program over csrc/levenberg.hpp for a sanitizer build (no GPU, no Python): the Cholesky solve and the accept / reject step
// at N = 6 and N = 7 on heap buffers of exact size -- a positive-definite system, a zero, a negative and a too-large pivot, an accepted and a
// rejected step against plain double arithmetic, ten rejections in a row and rho == 0.
//
//   hipcc -std=c++17 -O1 -g -ffp-contract=off --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined tools/levenberg_host_check.hip -o levenberg_host_check
//   ./levenberg_host_check           # prints the residual of the solve and "ok" for each N
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <memory>

#include "../structure-plp-slam_amd/csrc/levenberg.hpp"

using namespace plp;

template <int N, int E> struct Work {
    double est[E], bak[E], sum[N * (N + 1) / 2 + N + 1], x[N];
    double lambda, ni, current_chi, rho;
    int32_t ok2, qmax, rejected, go_on;
};

template <int N, int E> bool run() {
    constexpr int NH = N * (N + 1) / 2;
    std::unique_ptr<double[]> H(new double[NH]), b(new double[N]), Lf(new double[N * N]), y(new double[N]), x(new double[N]);
    auto fill = [&](double diag, double off) {
        for (int i = 0; i < N; ++i)
            for (int j = i; j < N; ++j) H[lev_h_index<N>(i, j)] = i == j ? diag + i : off / (1 + i + j);
        for (int i = 0; i < N; ++i) { b[i] = 1.0 - 0.25 * i; x[i] = 7.0; }
    };
    auto zero_x = [&] { bool z = true; for (int i = 0; i < N; ++i) z = z && x[i] == 0.0; return z; };
    // a positive-definite system: the residual of (H + lambda I) x = b
    const double lambda = 0.5;
    fill(4.0, 1.0);
    bool good = lev_chol<N>(H.get(), b.get(), lambda, Lf.get(), y.get(), x.get());
    double res = 0.0;
    for (int i = 0; i < N; ++i) {
        double r = -b[i];
        for (int j = 0; j < N; ++j) r += (H[i <= j ? lev_h_index<N>(i, j) : lev_h_index<N>(j, i)] + (i == j ? lambda : 0.0)) * x[j];
        res = std::fabs(r) > res ? std::fabs(r) : res;
    }
    good = good && res < 1e-12;
    // the last pivot zero, negative, above DBL_MAX (the first: DBL_MAX + DBL_MAX): false, x zero
    fill(4.0, 0.0); H[NH - 1] = -lambda;
    good = good && !lev_chol<N>(H.get(), b.get(), lambda, Lf.get(), y.get(), x.get()) && zero_x();
    fill(4.0, 0.0); H[NH - 1] = -1.0;
    good = good && !lev_chol<N>(H.get(), b.get(), lambda, Lf.get(), y.get(), x.get()) && zero_x();
    fill(4.0, 0.0); H[0] = kLevDblMax;
    good = good && !lev_chol<N>(H.get(), b.get(), kLevDblMax, Lf.get(), y.get(), x.get()) && zero_x();

    auto W = std::make_unique<Work<N, E>>();
    auto start = [&] {
        for (int i = 0; i < E; ++i) { W->est[i] = 1.0 + i; W->bak[i] = -1.0 - i; }
        for (int i = 0; i < NH + N + 1; ++i) W->sum[i] = 0.125 * (i % 5);
        for (int i = 0; i < N; ++i) W->x[i] = 0.01 * (i + 1);
        W->lambda = 0.75; W->ni = 2.0; W->current_chi = 10.0; W->rho = 0.0; W->ok2 = 1; W->qmax = 0; W->rejected = 0; W->go_on = 0;
    };
    auto scale_of = [&] {
        double s = 0.0;
        for (int j = 0; j < N; ++j) s = s + W->x[j] * (W->lambda * W->x[j] + W->sum[NH + j]);
        return s + 1e-3;
    };
    // an accepted step: the estimate stays, lambda shrinks by alpha cut to [1/3, 2/3]
    start();
    const double temp = 10.0 - 0.9 * scale_of();             // rho near 0.9: alpha lies inside the cut
    double rho = (10.0 - temp) / scale_of();
    double alpha = 1.0 - ((2.0 * rho - 1.0) * (2.0 * rho - 1.0)) * (2.0 * rho - 1.0);
    alpha = alpha < 2.0 / 3.0 ? alpha : 2.0 / 3.0;
    alpha = alpha > 1.0 / 3.0 ? alpha : 1.0 / 3.0;
    lev_decide_vertex<N, E>(*W, temp);
    good = good && alpha > 1.0 / 3.0 && alpha < 2.0 / 3.0 && W->rho == rho && W->lambda == 0.75 * alpha && W->ni == 2.0 && W->current_chi == temp &&
           W->est[E - 1] == 1.0 + (E - 1) && W->rejected == 0 && W->qmax == 1 && !W->go_on && lev_end(*W) == 0;
    // a rejected step, then nine more: the estimate goes back, lambda grows by ni = 2, 4, 8 ..., the tenth ends the iteration
    start();
    rho = (10.0 - 20.0) / scale_of();
    lev_decide_vertex<N, E>(*W, 20.0);
    good = good && W->rho == rho && W->lambda == 1.5 && W->ni == 4.0 && W->current_chi == 10.0 && W->est[E - 1] == -1.0 - (E - 1) && W->rejected == 1 && W->go_on == 1;
    double lam = 1.5, ni = 4.0;
    while (W->go_on) { lev_decide_vertex<N, E>(*W, 20.0); lam = lam * ni; ni = ni * 2.0; }
    good = good && W->qmax == kLevMaxTries && W->rejected == 10 && W->lambda == lam && W->ni == ni && lev_end(*W) == kLevEndTries;
    // a failed solve counts as DBL_MAX; rho == 0 is a rejection that ends the optimisation
    start(); W->ok2 = 0;
    lev_decide_vertex<N, E>(*W, 1.0);
    good = good && W->rho < 0.0 && W->rejected == 1 && W->go_on == 1;
    start();
    lev_decide_vertex<N, E>(*W, 10.0);
    good = good && W->rho == 0.0 && W->rejected == 1 && !W->go_on && W->lambda == 1.5 && lev_end(*W) == kLevEndRhoZero;
    // computeLambdaInit at iteration 0 only
    start(); W->sum[lev_h_index<N>(2, 2)] = -40.0; W->sum[NH + N] = 3.0;
    lev_begin<N>(*W, 0);
    good = good && W->lambda == 1e-5 * 40.0 && W->current_chi == 3.0 && W->qmax == 0;
    W->lambda = 9.0; lev_begin<N>(*W, 1);
    good = good && W->lambda == 9.0;
    std::printf("N = %d: residual %.3g, lambda after ten rejections %g: %s\n", N, res, lam, good ? "ok" : "FAILED");
    return good;
}

int main() { return run<6, 7>() && run<7, 8>() ? 0 : 1; }
