"""numpy restatement of gridhip_phase_shift and gridhip_average (include/gridhip.h, "phase shift and averaging"): the
definition the GPU tests compare against.  The phase is evaluated in np.longdouble, as dft_ref does, so the reference's own
error at |p| ~ 1e4 turns is far below the 1e-10 |vis| the tests allow; the coordinates are the rounded float64 expressions
of the header, which numpy reproduces to the bit.  The averaging is the integer rule with np.ldexp / np.rint and sums of
Python integers, which cannot round: bit for bit what the device must give."""
import numpy as np

TOL = 1e-10  # |vis' - ref| <= TOL |vis|: the DFT section's derivation for |p| <= 1e4 turns, one term
BIAS = 1084
CLASS_OF = (0, 0, 1, 1, 1, 2, 3)  # re, im | u, v, w | x | weight


def same_bits(a, b):
    """equal bit patterns, every NaN taken as the one NaN (x86 and the device differ in the sign of a generated NaN)"""
    def f64(v):
        v = np.ascontiguousarray(v)
        v = v.view(np.float64) if v.dtype == np.complex128 else v.astype(np.float64)
        return v.ravel().copy()
    a, b = f64(a), f64(b)
    if a.shape != b.shape:
        return False
    a[np.isnan(a)] = np.nan
    b[np.isnan(b)] = np.nan
    return np.array_equal(a.view(np.uint64), b.view(np.uint64))


def rotate_uvw(R, u, v, w):
    """(u', v', w'): every product rounded, the sums left to right"""
    R = np.asarray(R, dtype=np.float64).reshape(3, 3)
    with np.errstate(invalid="ignore", over="ignore"):
        return tuple((R[i, 0] * u + R[i, 1] * v) + R[i, 2] * w for i in range(3))


def phase_shift(R, u, v, w, vis):
    """-> (vis', (u', v', w'), bad) as gridhip_phase_shift defines them; bad: the visibilities with non-finite coordinates"""
    R = np.asarray(R, dtype=np.float64).reshape(3, 3)
    u, v = np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64)
    w = np.zeros_like(u) if w is None else np.asarray(w, dtype=np.float64)
    vis = np.asarray(vis, dtype=np.complex128)
    bad = ~(np.isfinite(u) & np.isfinite(v) & np.isfinite(w))
    L = np.longdouble
    l0, m0 = L(R[2, 0]), L(R[2, 1])
    r2 = l0 * l0 + m0 * m0
    nm1 = -r2 / (1 + np.sqrt(max(1 - r2, L(0))))
    uu, vv, ww = (np.where(bad, 0.0, a).astype(L) for a in (u, v, w))
    p = uu * l0 + vv * m0 + ww * nm1
    r = p - np.rint(p)
    ang = 2 * np.arctan2(L(0), L(-1)) * r
    c, s = np.cos(ang), np.sin(ang)
    re, im = vis.real.astype(L), vis.imag.astype(L)
    out = np.empty(len(vis), dtype=np.complex128)
    out.real, out.imag = (re * c - im * s).astype(np.float64), (re * s + im * c).astype(np.float64)
    out[bad] = vis[bad]
    return out, rotate_uvw(R, u, v, w), int(bad.sum())


def exponent_field(y):
    return ((np.ascontiguousarray(y, dtype=np.float64).view(np.uint64) >> np.uint64(52)) & np.uint64(0x7ff)).astype(np.int64)


def log2_ceil(n):
    return 0 if n <= 1 else (int(n) - 1).bit_length()


def integer_sum(cols, L=None):
    """The sums of one class of columns of one group: cols is a list of equally long float64 arrays of finite weighted
    values.  -> (sums as float64, one per column; s)"""
    n = len(cols[0])
    L = log2_ceil(n) if L is None else L
    b = max(int(exponent_field(c).max()) for c in cols)
    s = BIAS - L - b
    out = []
    for c in cols:
        q = np.rint(np.ldexp(np.asarray(c, dtype=np.float64), s))
        assert np.all(np.abs(q) <= 2.0 ** (62 - L))
        # exact: the upper and lower 32 bits are summed apart (neither sum can leave int64 for n < 2^31) and joined as
        # Python integers
        qi = q.astype(np.int64)
        Q = (int((qi >> 32).sum()) << 32) + int((qi & 0xffffffff).sum())
        assert abs(Q) < 2 ** 63
        with np.errstate(over="ignore", under="ignore"):
            out.append(np.ldexp(np.float64(float(Q)), -s))
    return out, s


def classes(group, G, y, wt):
    """0 participant, 1 flagged, 2 left out, 3 not finite: the first that applies"""
    cl = np.zeros(len(group), dtype=np.int64)
    fin = np.ones(len(group), dtype=bool)
    for c in y[:6]:
        fin &= np.isfinite(c)
    cl[~fin] = 3
    cl[(group < 0) | (group >= G)] = 2
    cl[~(wt > 0.0)] = 1
    return cl


def average(group, G, u, v, w, vis, x=None, wt=None, R=None):
    """-> (u_g, v_g, w_g, x_g, vis_g, wt_g, count, stats) as gridhip_average defines them.  With R the stream is first
    taken through this file's phase_shift (whose visibilities are NOT the device's bits: the fused form is compared on
    the device against the device's own phase_shift)."""
    u, v = np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64)
    n = len(u)
    w = np.zeros(n) if w is None else np.asarray(w, dtype=np.float64)
    vis = np.asarray(vis, dtype=np.complex128)
    xs = np.zeros(n) if x is None else np.asarray(x, dtype=np.float64)
    s = np.ones(n) if wt is None else np.asarray(wt, dtype=np.float64)
    group = np.zeros(n, dtype=np.int64) if group is None else np.asarray(group, dtype=np.int64)
    nbad = 0
    if R is not None:
        vis, (u, v, w), nbad = phase_shift(R, u, v, w, vis)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        y = [s * vis.real, s * vis.imag, s * u, s * v, s * w, s * xs, s.copy()]
    cl = classes(group, G, y, s)
    part = np.flatnonzero(cl == 0)
    order = part[np.argsort(group[part], kind="stable")]
    gs = group[order]
    out = np.zeros((7, G))
    count = np.zeros(G, dtype=np.int64)
    starts = np.flatnonzero(np.r_[True, gs[1:] != gs[:-1]]) if len(gs) else np.zeros(0, dtype=np.int64)
    ends = np.r_[starts[1:], len(gs)]
    for a, b in zip(starts, ends):
        g, idx = int(gs[a]), order[a:b]
        count[g] = len(idx)
        sums = [None] * 7
        for c in range(4):
            members = [j for j in range(7) if CLASS_OF[j] == c]
            vals, _ = integer_sum([y[j][idx] for j in members])
            for j, val in zip(members, vals):
                sums[j] = val
        W = sums[6]
        with np.errstate(invalid="ignore", over="ignore", under="ignore", divide="ignore"):
            out[:6, g] = [np.float64(t) / W for t in sums[:6]]
        out[6, g] = W
    stats = np.array([(count > 0).sum(), len(part), (cl == 1).sum(), (cl == 2).sum(), (cl == 3).sum(),
                      count.max() if G else 0, nbad, 0], dtype=np.float64)
    vis_g = np.empty(G, dtype=np.complex128)  # (not re + 1j * im: that loses a -0.0 and turns an Inf into a NaN)
    vis_g.real, vis_g.imag = out[0], out[1]
    return out[2], out[3], out[4], out[5], vis_g, out[6], count, stats
