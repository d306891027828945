"""numpy restatement of image-domain layers (include/gridhip.h, "w-stacking", IMAGE-DOMAIN LAYERS), built on
tests/wstack_ref.py (layers, screen, image_size) and oracle/gridref_np.py (ifft_c, fft_c, mirror_uvw, doweight).  Test
infrastructure, not product code.

The stack's planes, layers, centre planes and screens stay; only a layer's grid G_l is formed differently.  The
visibilities of one uv tile of T = Sg - K cells are summed as a direct Fourier sum, each with its exact residual w, onto an
Sg x Sg image (the subgrid), which is tapered, transformed and added to the grid; the taper is divided out of the image
inside the trusted region (the inner three quarters) and the image is 0 outside it.  The prediction is the exact adjoint."""
import numpy as np

import wstack_ref as W
from oracle import gridref_np as R

SUBGRIDS = (16, 24, 32)


def check(Sg, K):
    if Sg not in SUBGRIDS or K % 2 or not 4 <= K <= Sg // 2:
        raise ValueError(f"subgrid {Sg} must be 16, 24 or 32 and margin {K} even, 4 <= margin <= subgrid / 2")


def e(p):
    """exp(2 pi i p) of a phase in turns, reduced first: r = p - rint(p)"""
    p = np.asarray(p, dtype=np.float64)
    return np.exp(2j * np.pi * (p - np.rint(p)))


def tiles(x, N, Sg, K):
    """-> (keep, t, o, a) of cell coordinates x: keep where 0 <= x < N (NaN is dropped), the tile t = floor(x / T), taken
    as floor(x) div T (the same number, without the rounding of the quotient), the subgrid origin o = t T - K / 2 and
    a = x - (o + Sg / 2) in [-T / 2, T / 2); t, o, a are 0 where dropped"""
    x = np.asarray(x, dtype=np.float64)
    T = Sg - K
    keep = (x >= 0.0) & (x < np.float64(N))
    t = np.floor(np.where(keep, x, 0.0)).astype(np.int64) // T
    o = t * T - K // 2
    a = np.where(keep, np.where(keep, x, 0.0) - (o + Sg // 2), 0.0)
    return keep, t, o, a


def taper(f, K):
    """t(f) = exp(beta (sqrt(1 - 4 f^2) - 1)), beta = 1.15 K"""
    f = np.asarray(f, dtype=np.float64)
    return np.exp(1.15 * K * (np.sqrt(1.0 - 4.0 * f * f) - 1.0))


def correction1(N, K):
    """c(x) = 1 / t((x - N div 2) / N) where 8 |x - N div 2| <= 3 N, else 0"""
    d = np.arange(N, dtype=np.int64) - N // 2
    ok = 8 * np.abs(d) <= 3 * N
    return np.where(ok, 1.0 / taper(np.where(ok, d, 0) / np.float64(N), K), 0.0)


def correction(N, K):
    c = correction1(N, K)
    return c[:, None] * c[None, :]


def trusted(N):
    """the slice of the cells with 8 |x - N div 2| <= 3 N"""
    return slice(N // 2 - (3 * N) // 8, N // 2 + (3 * N) // 8 + 1)


class Stack:
    """binds (u, v, w) in wavelengths as given (no mirror, no weights), as wstack_ref.Stack does"""

    def __init__(self, theta, lam, u, v, w, wstep, M, Sg, K):
        check(Sg, K)
        self.theta, self.lam, self.wstep, self.M, self.Sg, self.K = theta, lam, int(wstep), int(M), Sg, K
        self.N = N = W.image_size(theta, lam)
        self.n = len(u)
        w = np.asarray(w, dtype=np.float64)
        x = np.float64(N) * (np.asarray(u, dtype=np.float64) / np.float64(lam)) + np.float64(N // 2)
        y = np.float64(N) * (np.asarray(v, dtype=np.float64) / np.float64(lam)) + np.float64(N // 2)
        kx, self.tx, self.ox, self.a = tiles(x, N, Sg, K)
        ky, self.ty, self.oy, self.b = tiles(y, N, Sg, K)
        self.lay = W.layers(w, wstep, M)
        self.keep = kx & ky & self.lay["finite"]
        self.dropped = int(self.n - self.keep.sum())
        layer = self.lay["layer"]
        self.dw = np.zeros(self.n)
        self.dw[self.keep] = w[self.keep] - (self.lay["pc"][layer[self.keep]] * self.wstep).astype(np.float64)
        self.occupied = [int(l) for l in np.unique(layer[self.keep])]
        self.f = (np.arange(Sg, dtype=np.float64) - Sg // 2) / Sg
        l = self.f * np.float64(theta)
        r2 = l[None, :] * l[None, :] + l[:, None] * l[:, None]
        self.ok = r2 < 1.0
        self.ph = 1.0 - np.sqrt(np.where(self.ok, 1.0 - r2, 1.0))
        t = taper(self.f, K)
        self.tap = t[:, None] * t[None, :]
        # Wm[p, i] = e(-(p - Sg/2) f_i) / Sg: Gs = Wm Pt Wm^T
        self.Wm = e(-np.outer(np.arange(Sg) - Sg // 2, self.f)) / Sg
        self.C = correction(N, K)

    def _screen(self, l):
        return W.screen(self.theta, self.N, float(int(self.lay["pc"][l]) * self.wstep))

    def _items(self, l):
        """the occupied tiles of layer l -> (oy, ox, indices)"""
        k = np.flatnonzero(self.keep & (self.lay["layer"] == l))
        key = self.ty[k] * (self.N + 1) + self.tx[k]
        for t in np.unique(key):
            idx = k[key == t]
            yield int(self.oy[idx[0]]), int(self.ox[idx[0]]), idx

    def _phase(self, idx):
        """a_k f_i + b_k f_j - dw_k ph[j][i], shape (len(idx), Sg, Sg)"""
        return (self.a[idx, None, None] * self.f[None, None, :] + self.b[idx, None, None] * self.f[None, :, None]
                - self.dw[idx, None, None] * self.ph[None, :, :])

    def _clip(self, o):
        """the subgrid cells [lo, hi) that lie on the grid, and their grid cells"""
        lo, hi = max(0, -o), min(self.Sg, self.N - o)
        return lo, hi, o + lo, o + hi

    def grid(self, l, vis):
        G = np.zeros((self.N, self.N), dtype=np.complex128)
        for oy, ox, idx in self._items(l):
            P = np.where(self.ok, np.einsum("k,kji->ji", vis[idx], e(self._phase(idx))), 0.0)
            Gs = self.Wm @ (P * self.tap) @ self.Wm.T
            ly, hy, gy0, gy1 = self._clip(oy)
            lx, hx, gx0, gx1 = self._clip(ox)
            G[gy0:gy1, gx0:gx1] += Gs[ly:hy, lx:hx]
        return G

    def dirty(self, vis):
        """C x D, D = sum_l S_l ifft_c(G_l), complex N x N"""
        vis = np.asarray(vis, dtype=np.complex128)
        D = np.zeros((self.N, self.N), dtype=np.complex128)
        for l in self.occupied:
            D += self._screen(l) * R.ifft_c(self.grid(l, vis))
        return self.C * D

    def image(self, vis):
        return np.real(self.dirty(vis))

    def predict(self, model, vis_sub=None):
        """the exact adjoint; a dropped visibility predicts exactly 0"""
        model = np.asarray(model, dtype=np.float64)
        pred = np.zeros(self.n, dtype=np.complex128)
        Sg = self.Sg
        for l in self.occupied:
            F = R.fft_c(np.conj(self._screen(l)) * self.C * model)
            for oy, ox, idx in self._items(l):
                patch = np.zeros((Sg, Sg), dtype=np.complex128)
                ly, hy, gy0, gy1 = self._clip(oy)
                lx, hx, gx0, gx1 = self._clip(ox)
                patch[ly:hy, lx:hx] = F[gy0:gy1, gx0:gx1]
                p = np.where(self.ok, (np.conj(self.Wm).T @ patch @ np.conj(self.Wm)) * self.tap, 0.0)
                # (the header fixes the device's order of this sum, j outer and i inner; its value is what is restated)
                pred[idx] = np.einsum("ji,kji->k", p, e(-self._phase(idx)))
        return pred if vis_sub is None else np.asarray(vis_sub, dtype=np.complex128) - pred


def do_imaging(theta, lam, u, v, w, vis, wstep, M, Sg, K):
    """wstack_ref.do_imaging with image-domain layers -> (image, psf, pmax)"""
    u1, v1, w1, vis1 = R.mirror_uvw(np.asarray(u), np.asarray(v), np.asarray(w), np.asarray(vis))
    N = W.image_size(theta, lam)
    wt = R.doweight(N, u1 / np.float64(lam), v1 / np.float64(lam), np.ones(len(u1), dtype=np.complex128))
    st = Stack(theta, lam, u1, v1, w1, wstep, M, Sg, K)
    img, psf = 2.0 * st.image(wt * vis1), 2.0 * st.image(wt)
    pmax = psf.max()
    return img / pmax, psf / pmax, pmax


def predict(theta, lam, u, v, w, model, wstep, M, Sg, K, vis_sub=None):
    return Stack(theta, lam, u, v, w, wstep, M, Sg, K).predict(model, vis_sub)
