// aw_degrid_check — gridding.hpp's awdegrid on one GPU: the adjoint identity against convgrid4 on a small generated
// stream, vdot(g, convgrid4(wk, ak, vis)) == vdot(awdegrid(conj wk, conj ak, g), vis); a visibility with an
// out-of-range w-bin predicts exactly 0; an empty antenna table is refused.
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstdlib>

#include "gridding.hpp"

using namespace gridding;

int main(int argc, char **argv)
{
    const Int N = 48, W = 3, Q = 2, S = 9, A = 4, n = argc > 1 ? atoll(argv[1]) : 1500;
    WKernels wk, wkc;
    wk.W = W; wk.Q = Q; wk.gh = wk.gw = S;
    wk.data.resize((size_t)W * Q * Q * S * S);
    for (size_t i = 0; i < wk.data.size(); ++i) wk.data[i] = {std::cos(0.37 * i), std::sin(0.11 * i)};
    AKernels ak, akc;
    ak.A = A; ak.S = S;
    ak.data.resize((size_t)A * S * S);
    for (size_t i = 0; i < ak.data.size(); ++i) ak.data[i] = {1.0 + 0.01 * (i % 7), 0.02 * (i % 5) - 0.03};
    wkc = wk;
    akc = ak;
    for (auto &x : wkc.data) x = std::conj(x);
    for (auto &x : akc.data) x = std::conj(x);
    BaseLines p;
    std::vector<Int> wb(n), a1(n), a2(n);
    std::vector<Visibility> vis(n);
    for (Int k = 0; k < n; ++k) {
        p.u.push_back(0.55 * std::sin(1.3 * k));  // (some footprints hang over the grid's edges)
        p.v.push_back(0.55 * std::cos(0.7 * k));
        p.w.push_back(0.0);
        wb[k] = k % W;
        a1[k] = k % A;
        a2[k] = (k / A) % A;
        vis[k] = {std::cos(0.1 * k), std::sin(0.2 * k)};
    }
    Matrix<Visibility> g(N, N);
    for (size_t i = 0; i < g.data.size(); ++i) g.data[i] = {std::sin(0.013 * i), std::cos(0.029 * i)};
    try {
        Backend be(0);
        const Matrix<Visibility> G = be.convgrid4(wk, ak, Matrix<Visibility>(N, N), p, wb, a1, a2, vis);
        const std::vector<Visibility> d = be.awdegrid(wkc, akc, g, p, wb, a1, a2);
        Visibility lhs = 0.0, rhs = 0.0;
        for (size_t i = 0; i < g.data.size(); ++i) lhs += std::conj(g.data[i]) * G.data[i];
        for (Int k = 0; k < n; ++k) rhs += std::conj(d[k]) * vis[k];
        std::printf("adjoint %.3e\n", std::abs(lhs - rhs) / std::abs(lhs));
        std::vector<Int> bad = wb;
        bad[0] = W;
        const std::vector<Visibility> z = be.awdegrid(wk, ak, g, p, bad, a1, a2);
        std::printf("dropped %d %d\n", (int)(z[0] == Visibility(0.0, 0.0)), (int)(z[1] != Visibility(0.0, 0.0)));
        AKernels none = ak;
        none.A = 0;
        try {
            be.awdegrid(wk, none, g, p, wb, a1, a2);
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
