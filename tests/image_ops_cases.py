"""Inputs that test_oracle.py (host) and test_gpu_image_ops.py (GPU) share: the vectors at which the operations either
side of the gridder take their edge branches.  No GPU, no oracle: plain numpy."""
from fractions import Fraction

import numpy as np

# the largest double below one half: floor(|x| + 0.5) rounds it to 1, libm round to 0
BELOW_HALF = 0.49999999999999994
WSTEPS = (1, 7, 2000)


def tie_vector(wstep):
    """Every tie of the w-bin rule round(w / wstep) for k = -9 .. 9 (w = k * wstep / 2, exact: both signs, 0.0 and -0.0),
    the doubles next to each tie on both sides, and +-BELOW_HALF * wstep where that product is exact."""
    ties = np.arange(-9, 10, dtype=np.float64) * float(wstep) / 2.0
    w = [ties, np.array([-0.0]), np.nextafter(ties, np.inf), np.nextafter(ties, -np.inf)]
    if Fraction(BELOW_HALF) * wstep == Fraction(BELOW_HALF * wstep):
        w.append(np.array([BELOW_HALF * wstep, -BELOW_HALF * wstep]))
    return np.concatenate(w)


# (npixFF, npixKern, qpx) whose extraction starts before the transformed far field: na/2 - qpx*(npixKern/2) < qpx - 1
WKERNEL_REFUSED = [(8, 8, 2), (16, 16, 2)]
