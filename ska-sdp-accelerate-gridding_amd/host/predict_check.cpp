// predict_check — gridding.hpp's predict / predict_aw on one GPU: the adjoint identity against the imaging functions
// on a small generated stream, sum(model * Re(ifft_c(imgfn(vis)))) == N^-2 Re(vdot(vis, predict(model))), for the
// simple and the aw kind; the residual form returns vis_sub - predict(model) exactly; an unknown kind is refused.
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstdlib>

#include "gridding.hpp"

using namespace gridding;

// sum(model * Re(ifft_c(g))) against N^-2 Re(vdot(vis, pred)), relative
static double adjoint_gap(Backend &be, const Matrix<F> &model, const Matrix<Visibility> &g,
                          const std::vector<Visibility> &vis, const std::vector<Visibility> &pred)
{
    const Matrix<Visibility> img = be.ifft(g);
    double lhs = 0.0, rhs = 0.0;
    for (size_t i = 0; i < model.data.size(); ++i) lhs += model.data[i] * img.data[i].real();
    for (size_t k = 0; k < vis.size(); ++k) rhs += (std::conj(vis[k]) * pred[k]).real();
    rhs /= (double)model.h * (double)model.h;
    return std::abs(lhs - rhs) / std::abs(lhs);
}

int main(int argc, char **argv)
{
    const F theta = 0.1;
    const Int lam = 490, N = gridhip_image_size(theta, lam), W = 3, Q = 2, S = 9, A = 4;  // N = 49: odd
    const Int n = argc > 1 ? atoll(argv[1]) : 1500;
    WKernels wk;
    wk.W = W; wk.Q = Q; wk.gh = wk.gw = S;
    wk.data.resize((size_t)W * Q * Q * S * S);
    for (size_t i = 0; i < wk.data.size(); ++i) wk.data[i] = {std::cos(0.37 * i), std::sin(0.11 * i)};
    AKernels ak;
    ak.A = A; ak.S = S;
    ak.data.resize((size_t)A * S * S);
    for (size_t i = 0; i < ak.data.size(); ++i) ak.data[i] = {1.0 + 0.01 * (i % 7), 0.02 * (i % 5) - 0.03};
    const std::vector<F> wbins = {-40.0, 0.0, 40.0};
    BaseLines p;
    std::vector<Int> a1(n), a2(n);
    std::vector<Visibility> vis(n);
    for (Int k = 0; k < n; ++k) {
        p.u.push_back(0.45 * lam * std::sin(1.3 * k));
        p.v.push_back(0.45 * lam * std::cos(0.7 * k));
        p.w.push_back(50.0 * std::sin(0.3 * k));
        a1[k] = k % A;
        a2[k] = (k / A) % A;
        vis[k] = {std::cos(0.1 * k), std::sin(0.2 * k)};
    }
    Matrix<F> model(N, N);
    for (size_t i = 0; i < model.data.size(); ++i) model.data[i] = std::sin(0.013 * i) + 0.5 * std::cos(0.029 * i);
    try {
        Backend be(0);
        const std::vector<Visibility> ps = be.predict(0, theta, lam, model, p);
        std::printf("adjoint_simple %.3e\n", adjoint_gap(be, model, be.simple_imaging(theta, lam, p, vis), vis, ps));
        const std::vector<Visibility> pa = be.predict_aw(theta, lam, wk, wbins, ak, model, p, a1, a2);
        std::printf("adjoint_aw %.3e\n",
                    adjoint_gap(be, model, be.aw_imaging(theta, lam, wk, wbins, ak, p, a1, a2, vis), vis, pa));
        const std::vector<Visibility> r = be.predict_aw(theta, lam, wk, wbins, ak, model, p, a1, a2, &vis);
        bool exact = true;
        for (Int k = 0; k < n; ++k) exact = exact && r[k] == Visibility(vis[k].real() - pa[k].real(), vis[k].imag() - pa[k].imag());
        std::printf("residual %d\n", (int)exact);
        try {
            be.predict(7, theta, lam, model, p);
            std::printf("error 0\n");
        } catch (const Error &e) {
            std::printf("error %d\n", e.code);
        }
    } catch (const Error &e) {
        std::fprintf(stderr, "gridhip: %s\n", e.what());
        return 1;
    }
    return 0;
}
