// aw_check — the aw entry points of gridding.hpp on one GPU: do_imaging with aw_imaging as the imaging function and
// the one-call aw_gridding, on a small generated stream; prints the peaks and an EINVAL check.
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "gridding.hpp"

using namespace gridding;

int main(int argc, char **argv)
{
    const double theta = 0.008, f = 1.0e8, c = 299792458.0;
    const Int lam = 8000, W = 3, Q = 2, S = 9, A = 4, n = argc > 1 ? atoll(argv[1]) : 2000;  // N = 64
    WKernels wk;
    wk.W = W; wk.Q = Q; wk.gh = wk.gw = S;
    wk.data.resize((size_t)W * Q * Q * S * S);
    for (size_t i = 0; i < wk.data.size(); ++i) wk.data[i] = {std::cos(0.37 * i) / S, std::sin(0.11 * i) / S};
    AKernels ak;
    ak.A = A; ak.S = S;
    ak.data.resize((size_t)A * S * S);
    for (size_t i = 0; i < ak.data.size(); ++i) ak.data[i] = {1.0 + 0.01 * (i % 7), 0.02 * (i % 5)};
    const std::vector<F> wbins = {-100.0, 0.0, 100.0};
    BaseLines uvw, uvw_m;
    std::vector<Int> a1(n), a2(n);
    std::vector<Visibility> vis(n);
    for (Int k = 0; k < n; ++k) {
        const double u = 0.4 * std::sin(1.3 * k) * lam, v = 0.4 * std::cos(0.7 * k) * lam, w = 120.0 * std::sin(0.5 * k);
        uvw.u.push_back(u); uvw.v.push_back(v); uvw.w.push_back(w);
        uvw_m.u.push_back(u * c / f); uvw_m.v.push_back(v * c / f); uvw_m.w.push_back(w * c / f);
        a1[k] = k % A;
        a2[k] = (k / A) % A;
        vis[k] = {std::cos(0.1 * k), std::sin(0.2 * k)};
    }
    try {
        Backend be(0);
        auto [img, psf, pmax] = be.do_imaging_aw(theta, lam, wk, wbins, ak, uvw, a1, a2, vis);
        F psf_peak = -1e300;
        for (F x : psf.data) psf_peak = x > psf_peak ? x : psf_peak;
        std::printf("do_imaging_aw %d %.17g %.17g\n", (int)img.h, pmax, psf_peak);
        auto [gimg, mx] = be.aw_gridding(theta, lam, f, wk, wbins, ak, uvw_m, a1, a2, vis);
        std::printf("aw_gridding %d %.17g\n", (int)gimg.h, mx);
        AKernels none = ak;
        none.S = 0;
        none.A = 0;
        try {
            be.aw_gridding(theta, lam, f, wk, wbins, none, uvw_m, a1, a2, vis);
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
