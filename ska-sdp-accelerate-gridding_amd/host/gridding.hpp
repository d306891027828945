// gridding.hpp — C++ host-side mirror of the reference's gridding interface over the C ABI.
//
// The reference's host language is Haskell (src/Gridding.hs); its toolchain is absent from the
// build image, so the host side above include/gridhip.h is offered in C++ (header-only) with the
// reference's names, argument order and meaning:
//
//   grid a p v                      src/Gridding.hs:95-98
//   convgrid gcf a p v              :153-157
//   convgrid2 gcf a p wbin v        :199-204
//   convgrid3/convgrid4 wkerns akerns a p index v   :246-252, :318-324
//   simple_imaging / conv_imaging / w_cache_imaging / aw_imaging   :84, :115, :399, :452
//   do_imaging theta lam uvw a1 a2 t f vis imgfn    :509-519 (do_imaging_aw: imgfn = aw_imaging)
//   predict / predict_aw: the way back, model image -> visibilities (absent from the reference)
//   clean: Hogbom CLEAN, the minor cycle between do_imaging and predict (absent from the reference)
//   msclean: multi-scale CLEAN, clean with components of several scales (absent from the reference)
//   mfclean: multi-term CLEAN, the minor cycle of wide-band imaging over T Taylor terms (absent from the reference)
//   jclean: joint CLEAN of P images of one sky - Stokes planes, channels - at shared positions (absent from the reference)
//   automask: the clean mask from the map itself - two levels, pruned, grown, accumulated (absent from the reference)
//   fit_beam / restore: the restoring beam of a PSF, and model * beam + residual (absent from the reference)
//   weights: natural, uniform and Briggs imaging weights with a taper and data weights (absent from the reference)
//   gaincal, apply_gains: per-antenna gains by StEFCal and their application (absent from the reference)
//   jonescal, apply_jones, stokes: 2x2 Jones matrices per antenna, their application, correlations <-> Stokes (likewise)
//   ddcal, dd_subtract: direction-dependent gains of D directions at once and the subtraction of directions
//   flag_residuals: robust per-group clipping of visibility residuals (absent from the reference)
//   dft_predict, components_from_image: the exact visibilities of a component list (absent from the reference)
//   find_sources: a map as a list of Gaussian components - islands, moments, the beam deconvolved (absent from the reference)
//   mosaic, reproject: images on other tangent planes brought onto one plane and combined (absent from the reference)
//   (phase shift and averaging, gridhip_phase_shift / gridhip_average, have no mirror here: the C ABI and the Python binding carry them)
//   aw_gridding                                     src/ImageDataset.hs:29-86 (after the HDF5 reads)
//   mirror_uvw, doweight, make_grid_hermitian, ifft, w_kernel, findClosest
//
// Error behaviour: the reference's functions are total on well-formed input and `error` otherwise;
// here every C-ABI failure is thrown as gridding::Error carrying gridhip_last_error().
// Arrays are std::vector in the layouts of SURVEY.md §8b (complex = std::complex<double>, grids
// row-major [y][x]); a Matrix carries its shape.
#pragma once
#include <complex>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <tuple>
#include <utility>
#include <vector>

#include "../../include/gridhip.h"

namespace gridding {

using F = double;                        // src/Types.hs:7
using Visibility = std::complex<double>; // src/Types.hs:16
using Int = int64_t;

struct Error : std::runtime_error {
    int code;
    Error(int c, const std::string &m) : std::runtime_error(m), code(c) {}
};

template <typename T>
struct Matrix {  // row-major [h][w]
    Int h = 0, w = 0;
    std::vector<T> data;
    Matrix() = default;
    Matrix(Int h_, Int w_, T fill = T()) : h(h_), w(w_), data((size_t)h_ * w_, fill) {}
    T &operator()(Int y, Int x) { return data[(size_t)y * w + x]; }
    const T &operator()(Int y, Int x) const { return data[(size_t)y * w + x]; }
};

struct BaseLines {  // Vector (F,F,F) as Accelerate stores it: three arrays
    std::vector<F> u, v, w;
    size_t size() const { return u.size(); }
};

struct Kernel {  // [Q][Q][gh][gw]
    Int Q = 0, gh = 0, gw = 0;
    std::vector<Visibility> data;
};
struct WKernels {  // [W][Q][Q][gh][gw]
    Int W = 0, Q = 0, gh = 0, gw = 0;
    std::vector<Visibility> data;
};
struct AKernels {  // [A][S][S]
    Int A = 0, S = 0;
    std::vector<Visibility> data;
};
struct KernelOptions {  // src/Gridding.hs:30-38 (the fields the w-kernel path reads)
    Int wstep = 2000, qpx = 0, npixFF = 0, npixKern = 0;
};

class Backend {  // plays the role of the (run, runN) pair of `Runners`, src/Gridding.hs:28
   public:
    explicit Backend(int device = 0)
    {
        int rc = gridhip_create(device, &ctx_);
        if (rc) throw Error(rc, std::string("gridhip_create: ") + gridhip_strerror(rc));
    }
    ~Backend() { gridhip_destroy(ctx_); }
    Backend(const Backend &) = delete;
    Backend &operator=(const Backend &) = delete;
    gridhip_ctx *raw() { return ctx_; }

    static const double *cd(const std::vector<Visibility> &v) { return reinterpret_cast<const double *>(v.data()); }
    static double *cd(std::vector<Visibility> &v) { return reinterpret_cast<double *>(v.data()); }
    void check(int rc) const
    {
        if (rc) throw Error(rc, gridhip_last_error(ctx_));
    }

    // ---- gridders: the destination grid `a` is copied, accumulated into and returned ----
    Matrix<Visibility> grid(Matrix<Visibility> a, const BaseLines &p, const std::vector<Visibility> &v)
    {
        check(gridhip_grid(ctx_, a.h, a.w, cd(a.data), (Int)v.size(), p.u.data(), p.v.data(), 1, cd(v)));
        return a;
    }
    Matrix<Visibility> convgrid(const Kernel &gcf, Matrix<Visibility> a, const BaseLines &p,
                                const std::vector<Visibility> &v)
    {
        check(gridhip_convgrid(ctx_, a.h, a.w, cd(a.data), (Int)v.size(), gcf.Q, gcf.gh, gcf.gw, cd(gcf.data),
                               p.u.data(), p.v.data(), 1, cd(v)));
        return a;
    }
    Matrix<Visibility> convgrid2(const WKernels &gcf, Matrix<Visibility> a, const BaseLines &p,
                                 const std::vector<Int> &wbin, const std::vector<Visibility> &v)
    {
        check(gridhip_convgrid2(ctx_, a.h, a.w, cd(a.data), (Int)v.size(), gcf.W, gcf.Q, gcf.gh, gcf.gw,
                                cd(gcf.data), p.u.data(), p.v.data(), 1, wbin.data(), cd(v)));
        return a;
    }
    std::vector<Visibility> degrid2(const WKernels &gcf, const Matrix<Visibility> &a, const BaseLines &p,
                                    const std::vector<Int> &wbin)
    {
        std::vector<Visibility> out(p.size());
        check(gridhip_degrid2(ctx_, a.h, a.w, cd(a.data), (Int)p.size(), gcf.W, gcf.Q, gcf.gh, gcf.gw, cd(gcf.data),
                              p.u.data(), p.v.data(), 1, wbin.data(), cd(out)));
        return out;
    }
    // index = (wbin, a1, a2) as three arrays
    Matrix<Visibility> convgrid4(const WKernels &wk, const AKernels &ak, Matrix<Visibility> a, const BaseLines &p,
                                 const std::vector<Int> &wbin, const std::vector<Int> &a1,
                                 const std::vector<Int> &a2, const std::vector<Visibility> &v)
    {
        check(gridhip_awgrid(ctx_, a.h, a.w, cd(a.data), (Int)v.size(), wk.W, wk.Q, wk.gh, ak.A, cd(wk.data),
                             cd(ak.data), p.u.data(), p.v.data(), 1, wbin.data(), a1.data(), a2.data(), cd(v)));
        return a;
    }
    // the gather twin of convgrid4 (the kernel it scatters, not conjugated again); index = (wbin, a1, a2)
    std::vector<Visibility> awdegrid(const WKernels &wk, const AKernels &ak, const Matrix<Visibility> &a,
                                     const BaseLines &p, const std::vector<Int> &wbin, const std::vector<Int> &a1,
                                     const std::vector<Int> &a2)
    {
        std::vector<Visibility> out(p.size());
        check(gridhip_awdegrid(ctx_, a.h, a.w, cd(a.data), (Int)p.size(), wk.W, wk.Q, wk.gh, ak.A, cd(wk.data),
                               cd(ak.data), p.u.data(), p.v.data(), 1, wbin.data(), a1.data(), a2.data(), cd(out)));
        return out;
    }
    Matrix<Visibility> convgrid3(const WKernels &wk, const AKernels &ak, Matrix<Visibility> a, const BaseLines &p,
                                 const std::vector<Int> &wbin, const std::vector<Int> &a1,
                                 const std::vector<Int> &a2, const std::vector<Visibility> &v)
    {
        return convgrid4(wk, ak, std::move(a), p, wbin, a1, a2, v);
    }

    // ---- imaging functions (uvw in wavelengths) ----
    Matrix<Visibility> simple_imaging(F theta, Int lam, const BaseLines &uvw, const std::vector<Visibility> &vis)
    {
        const Int N = gridhip_image_size(theta, lam);
        Matrix<Visibility> g(N, N);
        check(gridhip_simple_imaging(ctx_, theta, lam, (Int)vis.size(), uvw.u.data(), uvw.v.data(), 1, cd(vis),
                                     cd(g.data)));
        return g;
    }
    Matrix<Visibility> conv_imaging(const Kernel &kv, F theta, Int lam, const BaseLines &uvw,
                                    const std::vector<Visibility> &vis)
    {
        const Int N = gridhip_image_size(theta, lam);
        Matrix<Visibility> g(N, N);
        check(gridhip_conv_imaging(ctx_, kv.Q, kv.gh, kv.gw, cd(kv.data), theta, lam, (Int)vis.size(), uvw.u.data(),
                                   uvw.v.data(), 1, cd(vis), cd(g.data)));
        return g;
    }
    Matrix<Visibility> w_cache_imaging(const KernelOptions &ko, F theta, Int lam, const BaseLines &uvw,
                                       const std::vector<Visibility> &vis)
    {
        const Int N = gridhip_image_size(theta, lam);
        Matrix<Visibility> g(N, N);
        check(gridhip_w_cache_imaging(ctx_, ko.wstep, ko.qpx, ko.npixFF, ko.npixKern, theta, lam, (Int)vis.size(),
                                      uvw.u.data(), uvw.v.data(), uvw.w.data(), 1, cd(vis), cd(g.data)));
        return g;
    }
    Matrix<Visibility> aw_imaging(F theta, Int lam, const WKernels &wk, const std::vector<F> &wbins,
                                  const AKernels &ak, const BaseLines &uvw, const std::vector<Int> &a1,
                                  const std::vector<Int> &a2, const std::vector<Visibility> &vis)
    {
        const Int N = gridhip_image_size(theta, lam);
        Matrix<Visibility> g(N, N);
        check(gridhip_aw_imaging(ctx_, theta, lam, wk.W, wk.Q, wk.gh, ak.A, cd(wk.data), wbins.data(), cd(ak.data),
                                 (Int)vis.size(), uvw.u.data(), uvw.v.data(), uvw.w.data(), 1, a1.data(), a2.data(),
                                 cd(vis), cd(g.data)));
        return g;
    }

    // do_imaging with w_cache_imaging kernops as the imaging function -> (image, psf, pmax)
    std::tuple<Matrix<F>, Matrix<F>, F> do_imaging_w_cache(F theta, Int lam, const BaseLines &uvw,
                                                          const std::vector<Visibility> &vis,
                                                          const KernelOptions &ko)
    {
        const Int N = gridhip_image_size(theta, lam);
        Matrix<F> img(N, N), psf(N, N);
        F pmax = 0;
        check(gridhip_do_imaging(ctx_, 2, ko.wstep, ko.qpx, ko.npixFF, ko.npixKern, ko.npixKern, nullptr, theta, lam,
                                 (Int)vis.size(), uvw.u.data(), uvw.v.data(), uvw.w.data(), 1, cd(vis),
                                 img.data.data(), psf.data.data(), &pmax));
        return {std::move(img), std::move(psf), pmax};
    }
    // do_imaging with aw_imaging as the imaging function (:509-549, :452-478) -> (image, psf, pmax); uvw in
    // wavelengths, weights from the mirrored uvw, one kernel table per batch for both passes
    std::tuple<Matrix<F>, Matrix<F>, F> do_imaging_aw(F theta, Int lam, const WKernels &wk, const std::vector<F> &wbins,
                                                      const AKernels &ak, const BaseLines &uvw,
                                                      const std::vector<Int> &a1, const std::vector<Int> &a2,
                                                      const std::vector<Visibility> &vis)
    {
        const Int N = gridhip_image_size(theta, lam);
        Matrix<F> img(N, N), psf(N, N);
        F pmax = 0;
        check(gridhip_do_imaging_aw(ctx_, theta, lam, wk.W, wk.Q, wk.gh, ak.A, cd(wk.data), wbins.data(), cd(ak.data),
                                    (Int)vis.size(), uvw.u.data(), uvw.v.data(), uvw.w.data(), 1, a1.data(), a2.data(),
                                    cd(vis), img.data.data(), psf.data.data(), &pmax));
        return {std::move(img), std::move(psf), pmax};
    }
    // aw_gridding, src/ImageDataset.hs:54-77 -> (image, max pixel): uvw in METRES, f in Hz; weights from the
    // un-mirrored uvw; image = real . ifft . make_grid_hermitian of the aw grid, not normalised
    std::pair<Matrix<F>, F> aw_gridding(F theta, Int lam, F f, const WKernels &wk, const std::vector<F> &wbins,
                                        const AKernels &ak, const BaseLines &uvw_m, const std::vector<Int> &a1,
                                        const std::vector<Int> &a2, const std::vector<Visibility> &vis)
    {
        const Int N = gridhip_image_size(theta, lam);
        Matrix<F> img(N, N);
        F mx = 0;
        check(gridhip_aw_gridding(ctx_, theta, lam, f, wk.W, wk.Q, wk.gh, ak.A, cd(wk.data), wbins.data(), cd(ak.data),
                                  (Int)vis.size(), uvw_m.u.data(), uvw_m.v.data(), uvw_m.w.data(), 1, a1.data(),
                                  a2.data(), cd(vis), img.data.data(), &mx));
        return {std::move(img), mx};
    }
    std::tuple<Matrix<F>, Matrix<F>, F> do_imaging_simple(F theta, Int lam, const BaseLines &uvw,
                                                         const std::vector<Visibility> &vis)
    {
        const Int N = gridhip_image_size(theta, lam);
        Matrix<F> img(N, N), psf(N, N);
        F pmax = 0;
        check(gridhip_do_imaging(ctx_, 0, 0, 0, 0, 0, 0, nullptr, theta, lam, (Int)vis.size(), uvw.u.data(),
                                 uvw.v.data(), uvw.w.data(), 1, cd(vis), img.data.data(), psf.data.data(), &pmax));
        return {std::move(img), std::move(psf), pmax};
    }

    // ---- prediction: the adjoint of an imaging function applied to fft_c(model) (gridhip_predict) ----
    // model: the real N x N image (N = gridhip_image_size(theta, lam)); uvw in wavelengths, not mirrored.  kind 0
    // simple, 1 conv (kv), 2 w_cache (ko).  vis_sub given: vis_sub - prediction (the residual).
    std::vector<Visibility> predict(int kind, F theta, Int lam, const Matrix<F> &model, const BaseLines &uvw,
                                    const Kernel *kv = nullptr, const KernelOptions *ko = nullptr,
                                    const std::vector<Visibility> *vis_sub = nullptr)
    {
        check_model(theta, lam, model);
        std::vector<Visibility> out(uvw.size());
        Int wstep = 0, Q = 0, npixFF = 0, gh = 0, gw = 0;
        if (kv) Q = kv->Q, gh = kv->gh, gw = kv->gw;
        if (ko) wstep = ko->wstep, Q = ko->qpx, npixFF = ko->npixFF, gh = gw = ko->npixKern;
        check(gridhip_predict(ctx_, kind, wstep, Q, npixFF, gh, gw, kv ? cd(kv->data) : nullptr, theta, lam,
                              model.data.data(), (Int)uvw.size(), uvw.u.data(), uvw.v.data(),
                              uvw.w.empty() ? nullptr : uvw.w.data(), 1, vis_sub ? cd(*vis_sub) : nullptr, cd(out)));
        return out;
    }
    // the same for aw_imaging (:452-478): the gather twin of awdegrid with conj(wk), conj(ak)
    std::vector<Visibility> predict_aw(F theta, Int lam, const WKernels &wk, const std::vector<F> &wbins,
                                       const AKernels &ak, const Matrix<F> &model, const BaseLines &uvw,
                                       const std::vector<Int> &a1, const std::vector<Int> &a2,
                                       const std::vector<Visibility> *vis_sub = nullptr)
    {
        check_model(theta, lam, model);
        std::vector<Visibility> out(uvw.size());
        check(gridhip_predict_aw(ctx_, theta, lam, wk.W, wk.Q, wk.gh, ak.A, cd(wk.data), wbins.data(), cd(ak.data),
                                 model.data.data(), (Int)uvw.size(), uvw.u.data(), uvw.v.data(), uvw.w.data(), 1,
                                 a1.data(), a2.data(), vis_sub ? cd(*vis_sub) : nullptr, cd(out)));
        return out;
    }

    // ---- deconvolution: Hogbom CLEAN (gridhip_clean; include/gridhip.h, "deconvolution") ----
    // image and psf as do_imaging returns them; `model` is accumulated into (model = model + clean(...)) and `image`
    // becomes the residual, both in place.  Returns {iterations, final peak, its flat index, flux added}.
    struct CleanStats {
        F iterations, peak, index, flux;
    };
    CleanStats clean(Matrix<F> &image, const Matrix<F> &psf, Matrix<F> &model, F gain = 0.1, F threshold = 0.0,
                     Int niter = 100, Int border = 0, Int patch = 0)
    {
        if (image.h != image.w || psf.h != image.h || psf.w != image.w || model.h != image.h || model.w != image.w)
            throw Error(GRIDHIP_EINVAL, "clean: image, psf and model must be N x N");
        F st[4] = {0, 0, 0, 0};
        check(gridhip_clean(ctx_, image.h, psf.data.data(), image.data.data(), model.data.data(), gain, threshold, niter,
                            border, patch, st));
        return {st[0], st[1], st[2], st[3]};
    }

    // ---- multi-scale CLEAN (gridhip_msclean; include/gridhip.h, "multi-scale deconvolution") ----
    // clean with components of the given scales (cells, increasing from the delta scale 0, at most 6 and at most 32).
    // An empty bias is the default 1 - 0.6 a_s / a_max.
    struct MsCleanStats {
        F iterations, peak, index, last_scale, flux;
        F per_scale[6];
    };
    MsCleanStats msclean(Matrix<F> &image, const Matrix<F> &psf, Matrix<F> &model, const std::vector<F> &scales,
                         std::vector<F> bias = {}, F gain = 0.1, F threshold = 0.0, Int niter = 100, Int border = 0,
                         Int patch = 0)
    {
        if (image.h != image.w || psf.h != image.h || psf.w != image.w || model.h != image.h || model.w != image.w)
            throw Error(GRIDHIP_EINVAL, "msclean: image, psf and model must be N x N");
        if (bias.empty() && !scales.empty()) {
            F amax = scales[0];
            for (F a : scales) amax = a > amax ? a : amax;
            for (F a : scales) bias.push_back(amax > 0 ? 1 - 0.6 * a / amax : 1);
        }
        if (bias.size() != scales.size()) throw Error(GRIDHIP_EINVAL, "msclean: one bias per scale");
        F st[12] = {0};
        check(gridhip_msclean(ctx_, image.h, psf.data.data(), image.data.data(), model.data.data(), (Int)scales.size(),
                              scales.data(), bias.data(), gain, threshold, niter, border, patch, st));
        MsCleanStats out = {st[0], st[1], st[2], st[3], st[4], {st[6], st[7], st[8], st[9], st[10], st[11]}};
        return out;
    }

    // ---- multi-term CLEAN (gridhip_mfclean; include/gridhip.h, "wide-band imaging") ----
    // T Taylor terms, 1 <= T <= 4, as stacks of N x N planes: images [T][N][N] become the residuals and models [T][N][N]
    // are accumulated into, both in place; psfs holds the 2T - 1 spectral PSFs.  reason: 0 niter components taken,
    // 1 |peak| <= threshold, 2 nothing selectable, 3 singular Hessian.
    struct MfCleanStats {
        F iterations, peak, index;
        F flux[4];
        F reason;
    };
    MfCleanStats mfclean(Int N, Int T, std::vector<F> &images, const std::vector<F> &psfs, std::vector<F> &models,
                         F gain = 0.1, F threshold = 0.0, Int niter = 100, Int border = 0, Int patch = 0)
    {
        if (N < 1 || T < 1 || T > 4 || (Int)images.size() != T * N * N || (Int)models.size() != T * N * N ||
            (Int)psfs.size() != (2 * T - 1) * N * N)
            throw Error(GRIDHIP_EINVAL, "mfclean: images and models must be T x N x N, psfs (2T - 1) x N x N, T in 1 .. 4");
        F st[8] = {0};
        check(gridhip_mfclean(ctx_, N, T, psfs.data(), images.data(), models.data(), gain, threshold, niter, border, patch,
                              st));
        return {st[0], st[1], st[2], {st[3], st[4], st[5], st[6]}, st[7]};
    }

    // ---- joint CLEAN (gridhip_jclean; include/gridhip.h, "joint deconvolution") ----
    // P images of one sky, 1 <= P <= 8, as a stack of N x N planes, searched on one statistic - metric 0: the weighted
    // sum of the planes, 1: of their squares - and cleaned at shared positions: images [P][N][N] become the residuals
    // and models [P][N][N] are accumulated into, both in place; psfs holds one PSF for all planes or one per plane.  An
    // empty weights is 1 for every plane; an empty mask is none; sigma is the noise the nsigma term multiplies.
    // reason: 0 niter components taken, 1 the stop level, 2 nothing selectable, 3 no usable sigma.
    struct JCleanStats {
        F iterations, peak, index, level, reason, first_peak;
        F flux[8];
    };
    JCleanStats jclean(Int N, Int P, std::vector<F> &images, const std::vector<F> &psfs, std::vector<F> &models,
                       int metric = 1, const std::vector<F> &weights = {}, F gain = 0.1, F threshold = 0.0, Int niter = 100,
                       Int border = 0, Int patch = 0, const std::vector<uint8_t> &mask = {}, F nsigma = 0.0, F sigma = 0.0,
                       F peak_frac = 0.0)
    {
        if (N < 1 || P < 1 || P > 8 || (Int)images.size() != P * N * N || (Int)models.size() != P * N * N ||
            ((Int)psfs.size() != N * N && (Int)psfs.size() != P * N * N) ||
            (!weights.empty() && (Int)weights.size() != P) || (!mask.empty() && (Int)mask.size() != N * N))
            throw Error(GRIDHIP_EINVAL, "jclean: images and models must be P x N x N, psfs N x N or P x N x N, P in 1 .. 8, "
                                        "one weight per plane, the mask N x N bytes");
        F st[GRIDHIP_JCLEAN_STATS] = {0};
        check(gridhip_jclean(ctx_, N, P, (Int)psfs.size() / (N * N), psfs.data(), images.data(), models.data(),
                             weights.empty() ? nullptr : weights.data(), metric, gain, threshold, niter, border, patch,
                             mask.empty() ? nullptr : mask.data(), nsigma, &sigma, peak_frac, st));
        JCleanStats out = {st[0], st[1], st[2], st[3], st[4], st[5], {}};
        for (int p = 0; p < 8; ++p) out.flux[p] = st[8 + p];
        return out;
    }

    // ---- image statistics, masks and noise-based stop levels (gridhip_image_stats, gridhip_clean_auto,
    // gridhip_msclean_auto; include/gridhip.h, "image statistics", "masks and noise-based stop levels") ----
    // The lower median, the MAD and sigma = 1.4826 MAD of the finite cells inside `border` and `mask` (one byte per
    // cell, empty: every cell): exact order statistics.
    struct ImageStats {
        F n, median, mad, sigma, min, max, skipped;
    };
    ImageStats image_stats(const Matrix<F> &image, const std::vector<uint8_t> &mask = {}, Int border = 0)
    {
        if (image.h != image.w || (!mask.empty() && (Int)mask.size() != image.h * image.w))
            throw Error(GRIDHIP_EINVAL, "image_stats: image must be N x N and the mask N x N bytes");
        F st[8] = {0};
        check(gridhip_image_stats(ctx_, image.h, image.data.data(), mask.empty() ? nullptr : mask.data(), border, st));
        return {st[0], st[1], st[2], st[3], st[4], st[5], st[6]};
    }
    // clean / msclean under a mask (cells whose byte is 0 are never selected; empty: none), stopping at
    // T = max(threshold, nsigma * sigma, peak_frac * |first peak|).  reason: 0 niter components taken, 1 |peak| <= T,
    // 2 nothing selectable, 3 no usable sigma.
    struct AutoStop {
        F T, reason, first_peak;
    };
    CleanStats clean_auto(Matrix<F> &image, const Matrix<F> &psf, Matrix<F> &model, const std::vector<uint8_t> &mask,
                          F nsigma, F sigma, F peak_frac, AutoStop *why = nullptr, F gain = 0.1, F threshold = 0.0,
                          Int niter = 100, Int border = 0, Int patch = 0)
    {
        if (image.h != image.w || psf.h != image.h || psf.w != image.w || model.h != image.h || model.w != image.w ||
            (!mask.empty() && (Int)mask.size() != image.h * image.w))
            throw Error(GRIDHIP_EINVAL, "clean_auto: image, psf, model and mask must be N x N");
        F st[8] = {0};
        check(gridhip_clean_auto(ctx_, image.h, psf.data.data(), image.data.data(), model.data.data(), gain, threshold,
                                 niter, border, patch, mask.empty() ? nullptr : mask.data(), nsigma, &sigma, peak_frac, st));
        if (why) *why = {st[4], st[5], st[6]};
        return {st[0], st[1], st[2], st[3]};
    }
    MsCleanStats msclean_auto(Matrix<F> &image, const Matrix<F> &psf, Matrix<F> &model, const std::vector<F> &scales,
                              std::vector<F> bias, const std::vector<uint8_t> &mask, F nsigma, F sigma, F peak_frac,
                              AutoStop *why = nullptr, F gain = 0.1, F threshold = 0.0, Int niter = 100, Int border = 0,
                              Int patch = 0)
    {
        if (image.h != image.w || psf.h != image.h || psf.w != image.w || model.h != image.h || model.w != image.w ||
            (!mask.empty() && (Int)mask.size() != image.h * image.w))
            throw Error(GRIDHIP_EINVAL, "msclean_auto: image, psf, model and mask must be N x N");
        if (bias.empty() && !scales.empty()) {
            F amax = scales[0];
            for (F a : scales) amax = a > amax ? a : amax;
            for (F a : scales) bias.push_back(amax > 0 ? 1 - 0.6 * a / amax : 1);
        }
        if (bias.size() != scales.size()) throw Error(GRIDHIP_EINVAL, "msclean_auto: one bias per scale");
        F st[16] = {0};
        check(gridhip_msclean_auto(ctx_, image.h, psf.data.data(), image.data.data(), model.data.data(), (Int)scales.size(),
                                   scales.data(), bias.data(), gain, threshold, niter, border, patch,
                                   mask.empty() ? nullptr : mask.data(), nsigma, &sigma, peak_frac, st));
        if (why) *why = {st[12], st[13], st[14]};
        MsCleanStats out = {st[0], st[1], st[2], st[3], st[4], {st[6], st[7], st[8], st[9], st[10], st[11]}};
        return out;
    }

    // ---- auto-masking (gridhip_automask; include/gridhip.h, "auto-masking") ----
    // The mask of the islands of `image` above T_hi = max(thr_hi, nsigma_hi * sigma, peak_frac * peak) with at least
    // min_cells cells, each extended to the whole island above T_lo it lies in and grown by `grow` cells, OR-ed into
    // `mask` (N x N bytes, updated in place; bytes that are not 0 stay as they are).  reason: 0 the steps ran, 2 no cell
    // takes part, 3 no usable sigma (the mask is then untouched).
    struct AutomaskStats {
        F T_hi, T_lo, peak, components, surviving, kept, cells_set, reason;
    };
    AutomaskStats automask(const Matrix<F> &image, std::vector<uint8_t> &mask, F sigma, F nsigma_hi = 5, F nsigma_lo = 2.5,
                           F thr_hi = 0, F thr_lo = 0, F peak_frac = 0, Int min_cells = 1, Int grow = 0, Int border = 0,
                           bool absolute = false)
    {
        if (image.h != image.w || (Int)mask.size() != image.h * image.w)
            throw Error(GRIDHIP_EINVAL, "automask: image must be N x N and the mask N x N bytes");
        F st[8] = {0};
        check(gridhip_automask(ctx_, image.h, image.data.data(), mask.data(), border, absolute ? 1 : 0, thr_hi, thr_lo,
                               nsigma_hi, nsigma_lo, &sigma, peak_frac, min_cells, grow, st));
        return {st[0], st[1], st[2], st[3], st[4], st[5], st[6], st[7]};
    }

    // ---- restoring beam and restore (gridhip_fit_beam, gridhip_restore; include/gridhip.h, "restoring beam and restore") ----
    // The elliptical Gaussian exp(-(A dx^2 + 2 B dx dy + C dy^2)) fitted to the PSF's main lobe: FWHMs in cells (a cell
    // is theta / N radians), bpa in radians from +x towards +y.  ok is false, and the rest NaN, when the fit failed.
    struct Beam {
        F A, B, C, bmaj, bmin, bpa, ncells, ok;
    };
    Beam fit_beam(const Matrix<F> &psf, Int window = 8, F cut = 0.5)
    {
        if (psf.h != psf.w) throw Error(GRIDHIP_EINVAL, "fit_beam: psf must be N x N");
        F b[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        check(gridhip_fit_beam(ctx_, psf.h, psf.data.data(), window, cut, b));
        return {b[0], b[1], b[2], b[3], b[4], b[5], b[6], b[7]};
    }
    // model convolved with the beam over +-support cells (1 to 32) + residual, in units per beam
    Matrix<F> restore(const Matrix<F> &model, const Matrix<F> &residual, const Beam &beam, Int support)
    {
        if (model.h != model.w || residual.h != model.h || residual.w != model.w)
            throw Error(GRIDHIP_EINVAL, "restore: model and residual must be N x N");
        const F b[8] = {beam.A, beam.B, beam.C, beam.bmaj, beam.bmin, beam.bpa, beam.ncells, beam.ok};
        Matrix<F> out = residual;
        check(gridhip_restore(ctx_, model.h, model.data.data(), residual.data.data(), b, support, out.data.data()));
        return out;
    }

    // ---- imaging weights (gridhip_weights; include/gridhip.h, "imaging weights") ----
    enum class Weighting : int { natural = 0, uniform = 1, briggs = 2 };
    struct WeightStats {
        F sum_w, sum_w2_over_s, sum_s, noise, f2, n_used, n_flagged, n_outside;
    };
    // The weights of the baselines `uvw` (wavelengths, taken as given: mirror first for Hermitian cells) on the grid of
    // gridhip_image_size(theta, lam): robust is Briggs', taper_sigma a Gaussian taper in wavelengths (0: none), data the
    // data weights (empty: ones; a value that is not > 0 flags its visibility, whose weight is exactly 0).
    std::vector<F> weights(F theta, Int lam, const BaseLines &uvw, Weighting mode = Weighting::uniform, F robust = 0,
                           F taper_sigma = 0, const std::vector<F> &data = {}, WeightStats *stats = nullptr)
    {
        const Int n = (Int)uvw.u.size();
        if ((Int)uvw.v.size() != n || (!data.empty() && (Int)data.size() != n))
            throw Error(GRIDHIP_EINVAL, "weights: u, v and the data weights must hold one value per visibility");
        std::vector<F> out((size_t)n);
        F st[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        check(gridhip_weights(ctx_, theta, lam, n, uvw.u.data(), uvw.v.data(), 1, data.empty() ? nullptr : data.data(),
                              (int)mode, robust, taper_sigma, out.data(), st));
        if (stats) *stats = {st[0], st[1], st[2], st[3], st[4], st[5], st[6], st[7]};
        return out;
    }

    // ---- gain calibration (gridhip_gaincal, gridhip_apply_gains; include/gridhip.h, "gain calibration") ----
    // (Host forms, as everything in this class; the device-pointer forms gridhip_gaincal_dev, gridhip_apply_gains_dev and
    // the imager's gridhip_imager_selfcal_dev are the C header's, like every other _dev and imager entry point.)
    struct GainStats {
        F iterations, rel, chi2, chi2_unit, n_used, n_flagged, n_dropped, n_unsolved;
    };
    // The [T][A] antenna gains of vis ~ g[slot, a1] model conj(g[slot, a2]) by StEFCal, starting from 1 (or, warm, from
    // `gains`).  slot empty: one interval (T must be 1); data empty: ones, a value that is not > 0 flags its
    // visibility.  refant < 0: no rotation.  At most niter iterations, stopped once the relative change is <= tol.
    std::vector<Visibility> gaincal(const std::vector<Visibility> &vis, const std::vector<Visibility> &model,
                                    const std::vector<Int> &a1, const std::vector<Int> &a2, Int A,
                                    const std::vector<Int> &slot = {}, Int T = 1, const std::vector<F> &data = {},
                                    bool phase_only = false, Int refant = 0, Int niter = 50, F tol = 1e-8,
                                    GainStats *stats = nullptr, const std::vector<Visibility> *warm = nullptr)
    {
        const Int n = (Int)vis.size();
        if ((Int)model.size() != n || (Int)a1.size() != n || (Int)a2.size() != n || (!slot.empty() && (Int)slot.size() != n) ||
            (!data.empty() && (Int)data.size() != n) || A < 2 || T < 1 || (warm && (Int)warm->size() != A * T))
            throw Error(GRIDHIP_EINVAL, "gaincal: one value per visibility, A >= 2, T >= 1, gains of T x A");
        std::vector<Visibility> g = warm ? *warm : std::vector<Visibility>((size_t)(A * T));
        F st[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        check(gridhip_gaincal(ctx_, n, A, T, a1.data(), a2.data(), slot.empty() ? nullptr : slot.data(), cd(vis), cd(model),
                              data.empty() ? nullptr : data.data(), phase_only ? 1 : 0, refant, warm ? 1 : 0, niter, tol,
                              cd(g), st));
        if (stats) *stats = {st[0], st[1], st[2], st[3], st[4], st[5], st[6], st[7]};
        return g;
    }
    // vis after the [T][A] gains: inverse - data corrected, vis / (g_p conj(g_q)), *wt_out = data |g_p|^2 |g_q|^2 and 0 where
    // there is no usable gain; else a model corrupted, g_p vis conj(g_q), weights copied
    std::vector<Visibility> apply_gains(const std::vector<Visibility> &gains, Int A, Int T, const std::vector<Visibility> &vis,
                                        const std::vector<Int> &a1, const std::vector<Int> &a2,
                                        const std::vector<Int> &slot = {}, bool inverse = true,
                                        const std::vector<F> &data = {}, std::vector<F> *wt_out = nullptr)
    {
        const Int n = (Int)vis.size();
        if ((Int)a1.size() != n || (Int)a2.size() != n || (!slot.empty() && (Int)slot.size() != n) ||
            (!data.empty() && (Int)data.size() != n) || A < 2 || T < 1 || (Int)gains.size() != A * T)
            throw Error(GRIDHIP_EINVAL, "apply_gains: one value per visibility, gains of T x A");
        std::vector<Visibility> out((size_t)n);
        if (wt_out) wt_out->assign((size_t)n, 0);
        check(gridhip_apply_gains(ctx_, n, A, T, a1.data(), a2.data(), slot.empty() ? nullptr : slot.data(), cd(gains),
                                  inverse ? 1 : 0, cd(vis), data.empty() ? nullptr : data.data(), cd(out),
                                  wt_out ? wt_out->data() : nullptr));
        return out;
    }

    // ---- direction-dependent calibration (gridhip_ddcal, gridhip_dd_subtract; include/gridhip.h, "direction-dependent
    // calibration") ----
    // (Host forms; the device-pointer forms gridhip_ddcal_dev, gridhip_dd_subtract_dev and the imager's
    // gridhip_imager_peel_dev and the pure gridhip_ddcal_lds_antennas are the C header's.)
    // The [D][T][A] gains of vis ~ sum_d g[d, slot, a1] models[d] conj(g[d, slot, a2]), models [D][n] row after row, by the
    // multi-direction StEFCal.  The other arguments are gaincal's.
    std::vector<Visibility> ddcal(const std::vector<Visibility> &vis, const std::vector<Visibility> &models, Int D,
                                  const std::vector<Int> &a1, const std::vector<Int> &a2, Int A,
                                  const std::vector<Int> &slot = {}, Int T = 1, const std::vector<F> &data = {},
                                  bool phase_only = false, Int refant = 0, Int niter = 50, F tol = 1e-8,
                                  GainStats *stats = nullptr, const std::vector<Visibility> *warm = nullptr)
    {
        const Int n = (Int)vis.size();
        if (D < 1 || (Int)models.size() != D * n || (Int)a1.size() != n || (Int)a2.size() != n ||
            (!slot.empty() && (Int)slot.size() != n) || (!data.empty() && (Int)data.size() != n) || A < 2 || T < 1 ||
            (warm && (Int)warm->size() != D * A * T))
            throw Error(GRIDHIP_EINVAL, "ddcal: one value per visibility, D rows of models, A >= 2, T >= 1, gains of D x T x A");
        std::vector<Visibility> g = warm ? *warm : std::vector<Visibility>((size_t)(D * A * T));
        F st[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        check(gridhip_ddcal(ctx_, n, A, T, D, a1.data(), a2.data(), slot.empty() ? nullptr : slot.data(), cd(vis), cd(models),
                            data.empty() ? nullptr : data.data(), phase_only ? 1 : 0, refant, warm ? 1 : 0, niter, tol, cd(g),
                            st));
        if (stats) *stats = {st[0], st[1], st[2], st[3], st[4], st[5], st[6], st[7]};
        return g;
    }
    // vis (empty: zero, and the sign flips) minus the corrupted models of the directions in the bit set dirs
    std::vector<Visibility> dd_subtract(const std::vector<Visibility> &gains, Int D, Int A, Int T,
                                        const std::vector<Visibility> &models, const std::vector<Int> &a1,
                                        const std::vector<Int> &a2, const std::vector<Int> &slot, Int dirs,
                                        const std::vector<Visibility> &vis = {})
    {
        const Int n = (Int)a1.size();
        if (D < 1 || (Int)models.size() != D * n || (Int)a2.size() != n || (!slot.empty() && (Int)slot.size() != n) ||
            (!vis.empty() && (Int)vis.size() != n) || A < 2 || T < 1 || (Int)gains.size() != D * A * T)
            throw Error(GRIDHIP_EINVAL, "dd_subtract: one value per visibility, D rows of models, gains of D x T x A");
        std::vector<Visibility> out((size_t)n);
        check(gridhip_dd_subtract(ctx_, n, A, T, D, a1.data(), a2.data(), slot.empty() ? nullptr : slot.data(), cd(gains),
                                  cd(models), dirs, vis.empty() ? nullptr : cd(vis), cd(out)));
        return out;
    }

    // ---- polarisation (gridhip_jonescal, gridhip_apply_jones, gridhip_stokes; include/gridhip.h, "polarisation") ----
    // (Host forms; the device-pointer forms gridhip_jonescal_dev, gridhip_apply_jones_dev, gridhip_stokes_dev and the pure
    // gridhip_jonescal_lds_antennas are the C header's.)  A sample is four correlations, XX, XY, YX, YY one after the other:
    // vis and model hold 4 n values, gains 4 A T.
    enum class JonesMode { Full = 0, Diagonal = 1, Phase = 2 };
    // The [T][A][2][2] Jones matrices of vis ~ G[slot, a1] model G[slot, a2]^H by the matrix StEFCal, starting from the
    // identity (or, warm, from `gains`).  data: one weight per sample.  The other arguments are gaincal's.
    std::vector<Visibility> jonescal(const std::vector<Visibility> &vis, const std::vector<Visibility> &model,
                                     const std::vector<Int> &a1, const std::vector<Int> &a2, Int A,
                                     const std::vector<Int> &slot = {}, Int T = 1, const std::vector<F> &data = {},
                                     JonesMode mode = JonesMode::Full, Int refant = 0, Int niter = 50, F tol = 1e-8,
                                     GainStats *stats = nullptr, const std::vector<Visibility> *warm = nullptr)
    {
        const Int n = (Int)a1.size();
        if ((Int)vis.size() != 4 * n || (Int)model.size() != 4 * n || (Int)a2.size() != n ||
            (!slot.empty() && (Int)slot.size() != n) || (!data.empty() && (Int)data.size() != n) || A < 2 || T < 1 ||
            (warm && (Int)warm->size() != 4 * A * T))
            throw Error(GRIDHIP_EINVAL, "jonescal: four values per sample, A >= 2, T >= 1, gains of T x A x 2 x 2");
        std::vector<Visibility> g = warm ? *warm : std::vector<Visibility>((size_t)(4 * A * T));
        F st[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        check(gridhip_jonescal(ctx_, n, A, T, a1.data(), a2.data(), slot.empty() ? nullptr : slot.data(), cd(vis), cd(model),
                               data.empty() ? nullptr : data.data(), (int)mode, refant, warm ? 1 : 0, niter, tol, cd(g), st));
        if (stats) *stats = {st[0], st[1], st[2], st[3], st[4], st[5], st[6], st[7]};
        return g;
    }
    // vis after the [T][A][2][2] Jones matrices: inverse - data corrected, G_p^-1 vis G_q^-H, *wt_out = data |det G_p| |det G_q|
    // and 0 where there is no usable matrix; else a model corrupted, G_p vis G_q^H, weights copied
    std::vector<Visibility> apply_jones(const std::vector<Visibility> &gains, Int A, Int T, const std::vector<Visibility> &vis,
                                        const std::vector<Int> &a1, const std::vector<Int> &a2,
                                        const std::vector<Int> &slot = {}, bool inverse = true,
                                        const std::vector<F> &data = {}, std::vector<F> *wt_out = nullptr)
    {
        const Int n = (Int)a1.size();
        if ((Int)vis.size() != 4 * n || (Int)a2.size() != n || (!slot.empty() && (Int)slot.size() != n) ||
            (!data.empty() && (Int)data.size() != n) || A < 2 || T < 1 || (Int)gains.size() != 4 * A * T)
            throw Error(GRIDHIP_EINVAL, "apply_jones: four values per sample, gains of T x A x 2 x 2");
        std::vector<Visibility> out((size_t)(4 * n));
        if (wt_out) wt_out->assign((size_t)n, 0);
        check(gridhip_apply_jones(ctx_, n, A, T, a1.data(), a2.data(), slot.empty() ? nullptr : slot.data(), cd(gains),
                                  inverse ? 1 : 0, cd(vis), data.empty() ? nullptr : data.data(), cd(out),
                                  wt_out ? wt_out->data() : nullptr));
        return out;
    }
    // The [4][n] block of the Stokes rows I, Q, U, V of the four-correlation stream vis (4 n values); circular: the basis
    // is RR, RL, LR, LL.  which: the bit mask of the rows to write (I 1, Q 2, U 4, V 8); the others stay zero.
    std::vector<Visibility> stokes(const std::vector<Visibility> &vis, bool circular = false, int which = 15)
    {
        if (vis.size() % 4) throw Error(GRIDHIP_EINVAL, "stokes: four values per sample");
        std::vector<Visibility> v = vis, out(vis.size());
        check(gridhip_stokes(ctx_, (Int)(vis.size() / 4), circular ? 1 : 0, which, 0, cd(v), cd(out)));
        return out;
    }
    // The four-correlation stream (4 n values) of the [4][n] block of Stokes rows: how four per-Stokes predictions become
    // the model of jonescal
    std::vector<Visibility> stokes_inverse(const std::vector<Visibility> &iquv, bool circular = false)
    {
        if (iquv.size() % 4) throw Error(GRIDHIP_EINVAL, "stokes_inverse: four rows of n values");
        std::vector<Visibility> s = iquv, out(iquv.size());
        check(gridhip_stokes(ctx_, (Int)(iquv.size() / 4), circular ? 1 : 0, 15, 1, cd(out), cd(s)));
        return out;
    }

    // ---- residual flagging (gridhip_flag_residuals; include/gridhip.h, "residual flagging") ----
    // (Host form; the device-pointer forms gridhip_flag_residuals_dev and the imager's gridhip_imager_flag_dev are the C
    // header's.)
    struct FlagStats {
        F rounds, participants, clipped, not_finite, above_amax, left_alone, flagged_in, kept;
    };
    // The data weights of vis after clipping |vis - model| per group: the weight (1 where data is empty) of a sample that
    // is kept or left alone, +0.0 of one that is flagged.  model empty: zero; group empty: one group (G must be 1), else
    // group[k] in [0, G) and a sample outside is left alone.  T_g = median + nsigma * 1.4826 MAD per group and round; amax
    // > 0 also flags amplitudes above it.  flags: the class of every sample; group_stats: { n, median, MAD, T } per group.
    std::vector<F> flag_residuals(const std::vector<Visibility> &vis, const std::vector<Visibility> &model = {},
                                  const std::vector<Int> &group = {}, Int G = 1, const std::vector<F> &data = {},
                                  F nsigma = 5.0, F amax = 0.0, Int min_count = 8, Int niter = 3,
                                  std::vector<uint8_t> *flags = nullptr, std::vector<F> *group_stats = nullptr,
                                  FlagStats *stats = nullptr)
    {
        const Int n = (Int)vis.size();
        if ((!model.empty() && (Int)model.size() != n) || (!group.empty() && (Int)group.size() != n) ||
            (!data.empty() && (Int)data.size() != n) || G < 1 || (group.empty() && G != 1))
            throw Error(GRIDHIP_EINVAL, "flag_residuals: one value per visibility, G >= 1, a group array unless G == 1");
        std::vector<F> out((size_t)n);
        if (flags) flags->assign((size_t)n, 0);
        if (group_stats) group_stats->assign((size_t)(4 * G), 0);
        F st[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        check(gridhip_flag_residuals(ctx_, n, G, group.empty() ? nullptr : group.data(), cd(vis),
                                     model.empty() ? nullptr : cd(model), data.empty() ? nullptr : data.data(), nsigma, amax,
                                     min_count, niter, out.data(), flags ? flags->data() : nullptr,
                                     group_stats ? group_stats->data() : nullptr, st));
        if (stats) *stats = {st[0], st[1], st[2], st[3], st[4], st[5], st[6], st[7]};
        return out;
    }

    // ---- direct-Fourier prediction (gridhip_dft_predict, gridhip_components_from_image; include/gridhip.h) ----
    // (Host forms; the device-pointer forms are the C header's.)
    struct DftStats {
        F used, skipped, bad_vis, slices;
    };
    // The exact visibilities of the component rows {l, m, f0, f1, f2, f3, bmaj, bmin, bpa, 0} (comps: 10 doubles each) at
    // the baselines uvw (wavelengths, not mirrored; w empty: 0), or sub minus them.  x empty: x = 0; terms: how many of f0..f3 count.
    std::vector<Visibility> dft_predict(const std::vector<F> &comps, const BaseLines &uvw, Int terms = 1,
                                        const std::vector<F> &x = {}, const std::vector<Visibility> &sub = {},
                                        DftStats *stats = nullptr)
    {
        const Int n = (Int)uvw.size(), C = (Int)comps.size() / GRIDHIP_COMP_DOUBLES;
        if ((Int)comps.size() != C * GRIDHIP_COMP_DOUBLES || (Int)uvw.v.size() != n || (!uvw.w.empty() && (Int)uvw.w.size() != n) ||
            (!x.empty() && (Int)x.size() != n) || (!sub.empty() && (Int)sub.size() != n))
            throw Error(GRIDHIP_EINVAL, "dft_predict: 10 doubles per component, one v, w, x and sub per visibility");
        std::vector<Visibility> out((size_t)n);
        F st[4] = {0, 0, 0, 0};
        check(gridhip_dft_predict(ctx_, C, comps.data(), nullptr, (int)terms, n, uvw.u.data(), uvw.v.data(),
                                  uvw.w.empty() ? nullptr : uvw.w.data(), 1, x.empty() ? nullptr : x.data(),
                                  sub.empty() ? nullptr : cd(sub), cd(out), st));
        if (stats) *stats = {st[0], st[1], st[2], st[3]};
        return out;
    }
    // The non-zero cells of model[terms][N][N] as point components in row-major order: at most max_c rows; *found gets the
    // number of non-zero cells, which may exceed max_c
    std::vector<F> components_from_image(F theta, Int lam, Int terms, const std::vector<F> &model, Int max_c,
                                         Int *found = nullptr)
    {
        const Int N = gridhip_image_size(theta, lam);
        if (max_c < 0 || (Int)model.size() != terms * N * N)
            throw Error(GRIDHIP_EINVAL, "components_from_image: a model of terms x N x N, max_c >= 0");
        std::vector<F> comps((size_t)max_c * GRIDHIP_COMP_DOUBLES, 0);
        int64_t count = 0;
        check(gridhip_components_from_image(ctx_, theta, lam, (int)terms, model.data(), max_c, comps.data(), &count));
        comps.resize((size_t)(count < max_c ? count : max_c) * GRIDHIP_COMP_DOUBLES);
        if (found) *found = count;
        return comps;
    }

    // ---- source finding (gridhip_find_sources; include/gridhip.h, "source finding") ----
    // The islands of `image` (N x N, N = gridhip_image_size(theta, lam)) under automask's levels, without growing, each
    // measured by its moments and written as one component row {l, m, flux, 0, 0, 0, bmaj, bmin, bpa, 0} for dft_predict,
    // in ascending order of the island's first cell.  beam (fit_beam's; NULL: none) turns units per beam into integrated
    // flux and is deconvolved from the shape; correct undoes the cut of a Gaussian at T_lo.  At most max_c rows; info
    // (when given) receives GRIDHIP_SRC_DOUBLES doubles per row.  reason: 0 the steps ran, 2 no cell takes part, 3 no
    // usable sigma.
    struct SourceStats {
        F T_hi, T_lo, peak, found, written, points, flux, reason;
    };
    std::vector<F> find_sources(F theta, Int lam, const Matrix<F> &image, F sigma, Int max_c, const Beam *beam = nullptr,
                                bool correct = true, F nsigma_hi = 5, F nsigma_lo = 2.5, F thr_hi = 0, F thr_lo = 0,
                                F peak_frac = 0, Int min_cells = 1, Int border = 0, SourceStats *stats = nullptr,
                                std::vector<F> *info = nullptr)
    {
        const Int N = gridhip_image_size(theta, lam);
        if (max_c < 0 || image.h != N || image.w != N)
            throw Error(GRIDHIP_EINVAL, "find_sources: an image of N x N, N = image_size(theta, lam), max_c >= 0");
        std::vector<F> comps((size_t)max_c * GRIDHIP_COMP_DOUBLES, 0);
        if (info) info->assign((size_t)max_c * GRIDHIP_SRC_DOUBLES, 0);
        F b[8] = {0, 0, 0, 0, 0, 0, 0, 0}, st[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (beam) {
            const F v[8] = {beam->A, beam->B, beam->C, beam->bmaj, beam->bmin, beam->bpa, beam->ncells, beam->ok};
            for (int i = 0; i < 8; ++i) b[i] = v[i];
        }
        int64_t count = 0;
        check(gridhip_find_sources(ctx_, theta, lam, image.data.data(), border, thr_hi, thr_lo, nsigma_hi, nsigma_lo, &sigma,
                                   peak_frac, min_cells, beam ? b : nullptr, correct ? 1 : 0, max_c, comps.data(),
                                   info ? info->data() : nullptr, &count, st));
        const size_t rows = (size_t)(count < max_c ? count : max_c);
        comps.resize(rows * GRIDHIP_COMP_DOUBLES);
        if (info) info->resize(rows * GRIDHIP_SRC_DOUBLES);
        if (stats) *stats = {st[0], st[1], st[2], st[3], st[4], st[5], st[6], st[7]};
        return comps;
    }

    // ---- reprojection and mosaicking (gridhip_mosaic, gridhip_reproject; include/gridhip.h, "reprojection and mosaicking") ----
    // F facets of Ns x Ns cells (facets: F * Ns * Ns doubles, [f][y][x]; field of view theta_s) onto the Nd x Nd plane of
    // field of view theta_d.  R: 9 doubles per facet, the rotation from the destination frame to the facet's frame - what
    // phase_shift was given; kind 0 nearest, 1 bilinear, 3 cubic; inner, outer: the feather window in facet cells; weights
    // empty: none.  A facet whose R is no rotation with R22 > 0 is counted in stats and left out.
    struct MosaicStats {
        F covered, blank, used, refused, left_out, most, r6, r7;
    };
    Matrix<F> mosaic(Int F_, Int Ns, F theta_s, const std::vector<F> &facets, const std::vector<F> &R, Int Nd, F theta_d,
                     int kind, F inner, F outer, const std::vector<F> &weights = {}, bool normalize = true, F wmin = 0,
                     F blank = 0, Matrix<F> *wsum = nullptr, MosaicStats *stats = nullptr)
    {
        if (F_ < 1 || Ns < 1 || Nd < 1 || (Int)facets.size() != F_ * Ns * Ns || (Int)R.size() != F_ * 9 ||
            (!weights.empty() && weights.size() != facets.size()))
            throw Error(GRIDHIP_EINVAL, "mosaic: F x Ns x Ns facets, 9 doubles of R per facet, weights of the facets' shape");
        Matrix<F> out(Nd, Nd);
        if (wsum) *wsum = Matrix<F>(Nd, Nd);
        F st[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        check(gridhip_mosaic(ctx_, F_, Ns, theta_s, facets.data(), weights.empty() ? nullptr : weights.data(), R.data(), kind,
                             inner, outer, normalize ? 1 : 0, wmin, blank, Nd, theta_d, out.data.data(),
                             wsum ? wsum->data.data() : nullptr, st));
        if (stats) *stats = {st[0], st[1], st[2], st[3], st[4], st[5], st[6], st[7]};
        return out;
    }
    // the one-facet case: no weights, normalised; the way back from the full plane to a facet takes R^T
    Matrix<F> reproject(const Matrix<F> &image, F theta_s, const std::vector<F> &R, Int Nd, F theta_d, int kind, F inner,
                        F outer, F blank = 0)
    {
        if (image.h != image.w || image.h < 1 || Nd < 1 || R.size() != 9)
            throw Error(GRIDHIP_EINVAL, "reproject: a square image and the 9 doubles of one rotation");
        Matrix<F> out(Nd, Nd);
        check(gridhip_reproject(ctx_, image.h, theta_s, image.data.data(), R.data(), kind, inner, outer, blank, Nd, theta_d,
                                out.data.data()));
        return out;
    }

    // ---- helpers ----
    Matrix<Visibility> make_grid_hermitian(Matrix<Visibility> g)
    {
        check(gridhip_make_grid_hermitian(ctx_, g.h, cd(g.data)));
        return g;
    }
    Matrix<Visibility> ifft(const Matrix<Visibility> &m)
    {
        Matrix<Visibility> out(m.h, m.w);
        check(gridhip_fft2_centered(ctx_, m.h, cd(m.data), cd(out.data), 1));
        return out;
    }
    Kernel w_kernel(F theta, F w, const KernelOptions &ko)
    {
        Kernel k;
        k.Q = ko.qpx;
        k.gh = k.gw = ko.npixKern;
        k.data.resize((size_t)k.Q * k.Q * k.gh * k.gw);
        check(gridhip_w_kernel(ctx_, theta, w, ko.npixFF, ko.npixKern, ko.qpx, cd(k.data)));
        return k;
    }
    std::vector<Int> findClosest(const std::vector<F> &ws, const std::vector<F> &w)
    {
        std::vector<Int> out(w.size());
        check(gridhip_find_closest(ctx_, (Int)ws.size(), ws.data(), (Int)w.size(), w.data(), out.data()));
        return out;
    }

   private:
    gridhip_ctx *ctx_ = nullptr;
    static void check_model(F theta, Int lam, const Matrix<F> &model)
    {
        const Int N = gridhip_image_size(theta, lam);
        if (model.h != N || model.w != N) throw Error(GRIDHIP_EINVAL, "model must be N x N, N = gridhip_image_size(theta, lam)");
    }
};


// A whole node: visibility-sharded gridding over several GPUs of one process with one RCCL fp64 all-reduce of the
// partial grids (include/gridhip.h, gridhip_comm_*).  The reference has no counterpart (app/Main.hs:46-53 picks one
// (run, runN) pair); the signature stays convgrid2's.
class Node {
   public:
    explicit Node(int ndev, const int *dev_ids = nullptr)
    {
        int rc = gridhip_comm_create(ndev, dev_ids, &comm_);
        if (rc) throw Error(rc, std::string("gridhip_comm_create: ") + gridhip_comm_last_error(nullptr));
    }
    ~Node() { gridhip_comm_destroy(comm_); }
    Node(const Node &) = delete;
    Node &operator=(const Node &) = delete;
    int devices() const { return gridhip_comm_ndev(comm_); }

    Matrix<Visibility> convgrid2(const WKernels &gcf, Matrix<Visibility> a, const BaseLines &p,
                                 const std::vector<Int> &wbin, const std::vector<Visibility> &v)
    {
        int rc = gridhip_comm_convgrid2(comm_, a.h, a.w, reinterpret_cast<double *>(a.data.data()), (Int)v.size(), gcf.W,
                                        gcf.Q, gcf.gh, gcf.gw, reinterpret_cast<const double *>(gcf.data.data()),
                                        p.u.data(), p.v.data(), 1, wbin.data(), reinterpret_cast<const double *>(v.data()));
        if (rc) throw Error(rc, gridhip_comm_last_error(comm_));
        return a;
    }

   private:
    gridhip_comm *comm_ = nullptr;
};

}  // namespace gridding
