"""numpy restatement of an imager of the w-stacking kind (include/gridhip.h, "imagers", kind 4), built from
tests/wstack_ref.py's Stack and the oracle's mirror_uvw and doweight.  Test infrastructure, not product code.

The imager is defined by the two calls it replaces, gridhip_do_imaging_wstack and gridhip_predict_wstack:
    psf = 2 Re D(wt) / pmax, pmax = max(2 Re D(wt)), D on the MIRRORED stream;
    predict(model) on the UN-MIRRORED stream;
    cycle(model, vis).image = 2 Re D(wt conj-where-mirrored(vis - predict(model))) / pmax, vis_res = vis - predict(model).
wt is doweight's ones / count on the mirrored u / lam, v / lam, or the weights given (Context.weights' for the mirrored
stream); a weight that is not > 0 selects its visibility out, whatever its vis holds."""
import copy

import numpy as np

import wstack_ref as W
from oracle import gridref_np as R


def rebound(stack, u, v, w):
    """`stack` on another stream: the kernel table depends on neither the coordinates nor w, and is shared"""
    st = copy.copy(stack)
    st.pu = np.asarray(u, dtype=np.float64) / np.float64(stack.lam)
    st.pv = np.asarray(v, dtype=np.float64) / np.float64(stack.lam)
    st.n = len(st.pu)
    st.lay = W.layers(w, stack.wstep, stack.M)
    st.occupied = [int(l) for l in np.unique(st.lay["layer"]) if l >= 0]
    return st


class StackImager:
    def __init__(self, theta, lam, u, v, w, wstep, M, qpx, npixFF, npixKern, weights=None):
        u, v, w = (np.asarray(x, dtype=np.float64) for x in (u, v, w))
        self.N = W.image_size(theta, lam)
        self.neg = v < 0  # (-0.0 is not mirrored)
        u1, v1, w1, _ = R.mirror_uvw(u, v, w, np.zeros(len(u), dtype=np.complex128))
        if weights is None:
            weights = R.doweight(self.N, u1 / np.float64(lam), v1 / np.float64(lam), np.ones(len(u), dtype=np.complex128)).real
        self.wt = np.asarray(weights, dtype=np.float64)
        self.gather = W.Stack(theta, lam, u, v, w, wstep, M, qpx, npixFF, npixKern)  # predicts: the stream as given
        self.scatter = rebound(self.gather, u1, v1, w1)                               # images: the mirrored stream
        psf = 2.0 * self.scatter.image(self._weighted(np.ones(len(u), dtype=np.complex128)))
        self.pmax = psf.max() if len(u) else 0.0
        with np.errstate(invalid="ignore", divide="ignore"):
            self.psf = psf / self.pmax if len(u) else psf

    def _weighted(self, x):
        with np.errstate(invalid="ignore"):
            return np.where(self.wt > 0, self.wt * x, 0.0)

    def predict(self, model, vis_sub=None):
        return self.gather.predict(model, vis_sub)

    def cycle(self, vis, model=None):
        """-> (image, vis_res)"""
        vis = np.asarray(vis, dtype=np.complex128)
        r = vis if model is None else self.predict(model, vis)
        x = self._weighted(np.where(self.neg, np.conj(r), r))
        # (a visibility without a layer is not gridded, whatever x holds there: Stack.dirty visits occupied layers only)
        with np.errstate(invalid="ignore", divide="ignore"):
            return 2.0 * self.scatter.image(x) / self.pmax, r

