"""numpy restatement of w-stacking (include/gridhip.h, "w-stacking"), built from oracle/gridref_np.py's functions only:
acc_round, w_kernel, convgrid2, degrid2, ifft_c, fft_c, mirror_uvw and doweight.  Test infrastructure, not product code.

The w range is cut into layers of M planes of `wstep`.  A layer is gridded with the w-projection kernels of the residual
w alone (one table of M planes for all layers), transformed, multiplied by the exact w-screen of its centre plane and
summed; the prediction is the exact adjoint."""
import numpy as np

from oracle import gridref_np as R


def image_size(theta, lam):
    return R.haskell_round(theta * lam)


def layers(w, wstep, M):
    """-> dict(L, pmin, layer, r, pc, finite): the plane p = acc_round(w / wstep) of every visibility with a finite w,
    pmin / pmax over those, L = (pmax - pmin) div M + 1 layers, layer = (p - pmin) div M (-1 without a finite w), the
    centre planes pc[l] = pmin + l M + M div 2 and the residual bins r = p - pc[layer] + M div 2 in [0, M)."""
    w = np.asarray(w, dtype=np.float64)
    fin = np.isfinite(w)
    layer = np.full(len(w), -1, dtype=np.int64)
    r = np.zeros(len(w), dtype=np.int64)
    if not fin.any():
        return dict(L=0, pmin=0, layer=layer, r=r, pc=np.zeros(0, dtype=np.int64), finite=fin)
    p = np.zeros(len(w), dtype=np.int64)
    p[fin] = R.acc_round(w[fin] / np.float64(wstep))
    pmin, pmax = int(p[fin].min()), int(p[fin].max())
    L = (pmax - pmin) // M + 1
    layer[fin] = (p[fin] - pmin) // M
    pc = pmin + np.arange(L, dtype=np.int64) * M + M // 2
    r[fin] = p[fin] - pc[layer[fin]] + M // 2
    return dict(L=L, pmin=pmin, layer=layer, r=r, pc=pc, finite=fin)


def kernel_table(theta, wstep, M, npixFF, npixKern, qpx):
    """K[r] = conj(w_kernel(theta, (r - M div 2) wstep, ...)), r in [0, M): one table for all layers"""
    return np.stack([np.conj(R.w_kernel(theta, float((r - M // 2) * wstep), npixFF, npixKern, qpx)) for r in range(M)])


def screen(theta, N, wc, sign=-1.0):
    """S[y, x] = exp(sign 2 pi i wc ph[y, x]), ph = 1 - sqrt(1 - c_x^2 - c_y^2), c_i = (i - N div 2) / N theta; 0 where
    c_x^2 + c_y^2 >= 1.  sign = -1 is the screen of the stack (+1: for the test that tells the two apart)."""
    c = (np.arange(N, dtype=np.float64) - np.float64(N // 2)) / np.float64(N) * np.float64(theta)
    r2 = c[None, :] * c[None, :] + c[:, None] * c[:, None]
    ok = r2 < 1.0
    ph = 1.0 - np.sqrt(np.where(ok, 1.0 - r2, 1.0))
    return np.where(ok, np.exp(1j * (sign * 2.0 * np.pi * np.float64(wc) * ph)), 0.0)


class Stack:
    """The plan of the restatement: binds (u, v, w) in wavelengths as given (no mirror, no weights)."""

    def __init__(self, theta, lam, u, v, w, wstep, M, qpx, npixFF, npixKern, sign=-1.0):
        self.theta, self.lam, self.wstep, self.M, self.sign = theta, lam, int(wstep), int(M), sign
        self.N = image_size(theta, lam)
        self.pu = np.asarray(u, dtype=np.float64) / np.float64(lam)
        self.pv = np.asarray(v, dtype=np.float64) / np.float64(lam)
        self.n = len(self.pu)
        self.lay = layers(w, wstep, M)
        self.K = kernel_table(theta, wstep, M, npixFF, npixKern, qpx)
        self.occupied = [int(l) for l in np.unique(self.lay["layer"]) if l >= 0]

    def _screen(self, l):
        return screen(self.theta, self.N, float(int(self.lay["pc"][l]) * self.wstep), self.sign)

    def dirty(self, vis):
        """D = sum_l S_l ifft_c(G_l), complex N x N"""
        vis = np.asarray(vis, dtype=np.complex128)
        D = np.zeros((self.N, self.N), dtype=np.complex128)
        for l in self.occupied:
            k = self.lay["layer"] == l
            G = np.zeros((self.N, self.N), dtype=np.complex128)
            R.convgrid2(self.K, G, self.pu[k], self.pv[k], self.lay["r"][k], vis[k])
            D += self._screen(l) * R.ifft_c(G)
        return D

    def image(self, vis):
        return np.real(self.dirty(vis))

    def predict(self, model, vis_sub=None):
        """the exact adjoint, written at the visibility's own index; a visibility without a layer predicts exactly 0"""
        model = np.asarray(model, dtype=np.float64)
        pred = np.zeros(self.n, dtype=np.complex128)
        for l in self.occupied:
            k = self.lay["layer"] == l
            F = R.fft_c(np.conj(self._screen(l)) * model)
            pred[k] = R.degrid2(np.conj(self.K), F, self.pu[k], self.pv[k], self.lay["r"][k])
        return pred if vis_sub is None else np.asarray(vis_sub, dtype=np.complex128) - pred


def do_imaging(theta, lam, u, v, w, vis, wstep, M, qpx, npixFF, npixKern):
    """mirror, doweight on the mirrored u, v, one plan on the mirrored stream, image = 2 Re D(wt vis1), psf = 2 Re D(wt),
    both divided by pmax = max(psf) -> (image, psf, pmax)"""
    u1, v1, w1, vis1 = R.mirror_uvw(np.asarray(u), np.asarray(v), np.asarray(w), np.asarray(vis))
    N = image_size(theta, lam)
    wt = R.doweight(N, u1 / np.float64(lam), v1 / np.float64(lam), np.ones(len(u1), dtype=np.complex128))
    st = Stack(theta, lam, u1, v1, w1, wstep, M, qpx, npixFF, npixKern)
    img, psf = 2.0 * st.image(wt * vis1), 2.0 * st.image(wt)
    pmax = psf.max()
    return img / pmax, psf / pmax, pmax


def predict(theta, lam, u, v, w, model, wstep, M, qpx, npixFF, npixKern, vis_sub=None):
    return Stack(theta, lam, u, v, w, wstep, M, qpx, npixFF, npixKern).predict(model, vis_sub)
