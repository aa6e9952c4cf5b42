"""The matching filter of source-wavelet estimation restated in float64 numpy: the definitions the kernels of
csrc/mifwi_stf.hip and misfit.solve_matching_filter are tested against, and the error bounds that follow from them.

Traces are [nt, nshot, nrec]; a filter is [nshot, nlag], index i holds lag k = i - lag_before; terms whose time index
falls outside [0, nt) are absent."""
import numpy as np

U64 = 2.0 ** -52
U32 = 2.0 ** -24


def _shifted(x, k):
    """z[t] = x[t - k] where 0 <= t - k < nt, else 0 (float64)."""
    nt = x.shape[0]
    z = np.zeros(x.shape)
    lo, hi = max(0, k), min(nt, nt + k)
    if lo < hi:
        z[lo:hi] = x[lo - k:hi - k]
    return z


def convolve(x, h, lag_before, transpose=False, absolute=False):
    """y[t,s,r] = sum_i h[s,i] x[t-k,s,r] (transpose: x[t+k]); ``absolute``: sum_i |h[s,i]| |x[t-k,s,r]| instead."""
    x = np.asarray(x, dtype=np.float64)
    h = np.asarray(h, dtype=np.float64)
    if absolute:
        x, h = np.abs(x), np.abs(h)
    y = np.zeros(x.shape)
    for i in range(h.shape[1]):
        k = i - lag_before
        y += h[:, i][None, :, None] * _shifted(x, -k if transpose else k)
    return y


def correlations(pred, obs, lag_before, lag_after, w=None, absolute=False):
    """a[s,j] = sum_r w^2 sum_t x[t] x[t+j], c[s,i] = sum_r w^2 sum_t d[t] x[t-k]; a trace with w == 0 is not read.
    ``absolute``: the same sums of |.| |.| (what the rounding-error bound of the kernel is made of)."""
    x = np.array(pred, dtype=np.float64)
    d = np.array(obs, dtype=np.float64)
    nlag = lag_before + lag_after + 1
    w2 = np.ones(x.shape[1:]) if w is None else np.asarray(w, dtype=np.float64) ** 2
    dead = w2 == 0
    x[:, dead] = 0.0
    d[:, dead] = 0.0
    if absolute:
        x, d = np.abs(x), np.abs(d)
    a = np.zeros((x.shape[1], nlag))
    c = np.zeros((x.shape[1], nlag))
    for j in range(nlag):
        a[:, j] = (w2[None] * x * _shifted(x, -j)).sum(axis=(0, 2))
    for i in range(nlag):
        c[:, i] = (w2[None] * d * _shifted(x, i - lag_before)).sum(axis=(0, 2))
    return a, c


def toeplitz(a, water_level):
    """T[i,j] = a[|i-j|] + water_level a[0] (i == j) of one shot's autocorrelation."""
    n = len(a)
    idx = np.abs(np.arange(n)[:, None] - np.arange(n)[None, :])
    return a[idx] + water_level * a[0] * np.eye(n)


def solve(a, c, water_level, lag_before=0, per_shot=True):
    a, c = np.asarray(a, dtype=np.float64), np.asarray(c, dtype=np.float64)
    ns = a.shape[0]
    if not per_shot:
        a, c = a.sum(0, keepdims=True), c.sum(0, keepdims=True)
    h = np.zeros(c.shape)
    for s in range(a.shape[0]):
        if a[s, 0] == 0:
            h[s, lag_before] = 1.0
        else:
            h[s] = np.linalg.solve(toeplitz(a[s], water_level), c[s])
    return h if per_shot else np.repeat(h, ns, axis=0)


def estimate(pred, obs, lag_before, lag_after, water_level, w=None, per_shot=True):
    a, c = correlations(pred, obs, lag_before, lag_after, w)
    return solve(a, c, water_level, lag_before, per_shot)


def correlation_bound(pred, obs, lag_before, lag_after, w=None):
    """|a - a64|, |c - c64| <= nt nrec 2^-52 sum w^2 |x| |x'|: the products are exact in double, the sums have at most
    nt nrec terms each."""
    nt, _, nrec = np.shape(pred)
    aa, ca = correlations(pred, obs, lag_before, lag_after, w, absolute=True)
    return nt * nrec * U64 * aa, nt * nrec * U64 * ca


def convolve_bound(x, h, lag_before, transpose=False):
    """|y - y64| <= (nlag + 1) 2^-24 sum_i |h_i| |x_{t-k}|: the worst case of a float dot product of length nlag."""
    return (np.shape(h)[1] + 1) * U32 * convolve(x, h, lag_before, transpose, absolute=True)


def filter_bound(a, c, da, dc, water_level, h):
    """First-order perturbation of T h = c per shot: |dh|_2 <= 2 |T^-1|_2 (|dc|_2 + |dT|_2 |h|_2), dT the Toeplitz matrix
    of the bounds da (its 2-norm taken of the matrix of bounds, which dominates every admissible perturbation)."""
    out = np.zeros(a.shape[0])
    for s in range(a.shape[0]):
        if a[s, 0] == 0:
            continue
        tinv = np.linalg.norm(np.linalg.inv(toeplitz(a[s], water_level)), 2)
        dt = np.linalg.norm(toeplitz(da[s], water_level), 2)
        out[s] = 2.0 * tinv * (np.linalg.norm(dc[s]) + dt * np.linalg.norm(h[s]))
    return out
