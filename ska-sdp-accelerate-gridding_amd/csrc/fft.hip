// The transform: hipFFT, loaded on first use so the gridder itself has no dependency on it; the context's cache of four
// N x N Z2Z plans, plans a caller owns, and the centred transform built on them.  No other file names hipFFT.
#include <dlfcn.h>

#include "common.h"
#include "imaging.h"

namespace gridhip {

typedef int (*fn_plan2d)(void **, int, int, int);
typedef int (*fn_setstream)(void *, hipStream_t);
typedef int (*fn_exec)(void *, void *, void *, int);
typedef int (*fn_destroy)(void *);
static struct {
    void *h = nullptr;
    fn_plan2d plan2d;
    fn_setstream setstream;
    fn_exec exec;
    fn_destroy destroy;
    bool tried = false;
} g_fft;

static int load_hipfft(gridhip_ctx *ctx)
{
    if (g_fft.h) return GRIDHIP_OK;
    if (!g_fft.tried) {
        g_fft.tried = true;
        const char *names[] = {"libhipfft.so.0", "libhipfft.so", "/opt/rocm/lib/libhipfft.so"};
        for (const char *nm : names) {
            g_fft.h = dlopen(nm, RTLD_NOW | RTLD_GLOBAL);
            if (g_fft.h) break;
        }
        if (g_fft.h) {
            g_fft.plan2d = (fn_plan2d)dlsym(g_fft.h, "hipfftPlan2d");
            g_fft.setstream = (fn_setstream)dlsym(g_fft.h, "hipfftSetStream");
            g_fft.exec = (fn_exec)dlsym(g_fft.h, "hipfftExecZ2Z");
            g_fft.destroy = (fn_destroy)dlsym(g_fft.h, "hipfftDestroy");
            if (!g_fft.plan2d || !g_fft.setstream || !g_fft.exec || !g_fft.destroy) {
                dlclose(g_fft.h);
                g_fft.h = nullptr;
            }
        }
    }
    if (!g_fft.h) return fail(ctx, GRIDHIP_EHIP, "cannot load libhipfft.so: %s", dlerror());
    return GRIDHIP_OK;
}

// the context's cached N x N Z2Z plan, bound to its stream
int fft_plan_for(gridhip_ctx *ctx, int64_t N, void **out_plan)
{
    GH_CHECK(load_hipfft(ctx));
    if (N > 0x7fffffff) return fail(ctx, GRIDHIP_EUNSUPPORTED, "fft size");
    void *plan = nullptr;
    for (int i = 0; i < 4; ++i)
        if (ctx->img->fft_plan[i] && ctx->img->fft_n[i] == N) plan = ctx->img->fft_plan[i];
    if (!plan) {
        const int slot = ctx->img->fft_next;
        if (ctx->img->fft_plan[slot]) {
            // (a plan may still be in use by work queued on the stream)
            GH_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
            g_fft.destroy(ctx->img->fft_plan[slot]);
        }
        ctx->img->fft_plan[slot] = nullptr;
        int rc = g_fft.plan2d(&plan, (int)N, (int)N, 0x69 /* HIPFFT_Z2Z */);
        if (rc) return fail(ctx, GRIDHIP_EHIP, "hipfftPlan2d(%lld) failed: %d", (long long)N, rc);
        ctx->img->fft_plan[slot] = plan;
        ctx->img->fft_n[slot] = N;
        ctx->img->fft_next = (slot + 1) % 4;
    }
    if (int rc = g_fft.setstream(plan, ctx->stream)) return fail(ctx, GRIDHIP_EHIP, "hipfftSetStream: %d", rc);
    *out_plan = plan;
    return GRIDHIP_OK;
}

// a transform of the caller's own (an imager keeps one: the context's four cached sizes come and go with other calls)
int fft_plan_own(gridhip_ctx *ctx, int64_t N, void **out_plan)
{
    GH_CHECK(load_hipfft(ctx));
    if (N > 0x7fffffff) return fail(ctx, GRIDHIP_EUNSUPPORTED, "fft size");
    *out_plan = nullptr;
    if (int rc = g_fft.plan2d(out_plan, (int)N, (int)N, 0x69 /* HIPFFT_Z2Z */)) {
        *out_plan = nullptr;
        return fail(ctx, GRIDHIP_EHIP, "hipfftPlan2d(%lld) failed: %d", (long long)N, rc);
    }
    return GRIDHIP_OK;
}

int fft_plan_bind(gridhip_ctx *ctx, void *plan)
{
    if (int rc = g_fft.setstream(plan, ctx->stream)) return fail(ctx, GRIDHIP_EHIP, "hipfftSetStream: %d", rc);
    return GRIDHIP_OK;
}

void fft_plan_drop(void *plan)
{
    if (plan && g_fft.h) g_fft.destroy(plan);
}

int fft_exec(gridhip_ctx *ctx, void *plan, double2 *data, bool inverse)
{
    if (int rc = g_fft.exec(plan, data, data, inverse ? 1 /* HIPFFT_BACKWARD */ : -1 /* HIPFFT_FORWARD */))
        return fail(ctx, GRIDHIP_EHIP, "hipfftExecZ2Z: %d", rc);
    return GRIDHIP_OK;
}

// centred transform (src/Gridding.hs:815-829): shift2D . fft2D mode . ishift2D.
// accelerate-fft: Forward = exp(-i..) unnormalised, Inverse = exp(+i..) scaled by 1/N^2.
// `in` is preserved, `tmp` and `out` are N*N scratch/output (out may not alias in).
int dev_fft2c(gridhip_ctx *ctx, int64_t N, const double2 *in, double2 *out, double2 *tmp, bool inverse)
{
    void *plan = nullptr;
    GH_CHECK(fft_plan_for(ctx, N, &plan));
    GH_CHECK(launch_roll(ctx, N, in, tmp, N / 2, 1.0));
    GH_CHECK(fft_exec(ctx, plan, tmp, inverse));
    return launch_roll(ctx, N, tmp, out, (N + 1) / 2, inverse ? 1.0 / ((double)N * (double)N) : 1.0);
}

void fft_release(gridhip_ctx *ctx)
{
    if (ctx->img->wk_cache.ptr) (void)hipFree(ctx->img->wk_cache.ptr);
    ctx->img->wk_cache.ptr = nullptr;
    ctx->img->wk_cache.bytes = 0;
    ctx->img->wk_cache.nplanes = 0;
    for (int i = 0; i < 4; ++i) {
        if (ctx->img->fft_plan[i] && g_fft.h) g_fft.destroy(ctx->img->fft_plan[i]);
        ctx->img->fft_plan[i] = nullptr;
    }
}

}  // namespace gridhip
