"""Float64 numpy definition of the envelope objective (misfit.envelope, csrc/mifwi_envelope.hip): test infrastructure only.

Traces are [nt, ...], time on axis 0.  H is the Hilbert transform through a zero-padded DFT of N = the smallest power
of two >= nt points: bins 0 < k < N/2 times -i, N/2 < k < N times +i, bins 0 and N/2 times 0, inverse DFT, real part of
the first nt samples - scipy.signal.hilbert(x, N=N, axis=0).imag[:nt].  The multiplier is antisymmetric: H^T = -H."""
import numpy as np


def padded_length(nt):
    n = 1
    while n < nt:
        n *= 2
    return n


def hilbert(x, transpose=False):
    x = np.asarray(x, dtype=np.float64)
    nt = x.shape[0]
    n = padded_length(nt)
    k = np.arange(n)
    mult = np.where((k > 0) & (k < n / 2), -1j, 0) + np.where(k > n / 2, 1j, 0)
    spec = np.fft.fft(x, n=n, axis=0) * mult.reshape((n,) + (1,) * (x.ndim - 1))
    y = np.fft.ifft(spec, axis=0).real[:nt]
    return -y if transpose else y


def envelope(x, eps):
    x = np.asarray(x, dtype=np.float64)
    return np.sqrt(x * x + hilbert(x) ** 2 + float(eps) ** 2)


def loss_adj(s, o, eps):
    """loss = 1/2 sum (E(s) - E(o))**2 and adj = dloss/ds = r s / E(s) - H(r H(s) / E(s)); a term whose divisor E(s) is 0
    (possible with eps == 0 only) contributes 0."""
    s = np.asarray(s, dtype=np.float64)
    h = hilbert(s)
    es = np.sqrt(s * s + h * h + float(eps) ** 2)
    r = es - envelope(o, eps)
    live = es > 0
    safe = np.where(live, es, 1.0)
    a = np.where(live, r * s / safe, 0.0)
    q = np.where(live, r * h / safe, 0.0)
    return 0.5 * float((r * r).sum()), a - hilbert(q)


def ricker(nt, centre, freq):
    """Ricker wavelet of peak frequency ``freq`` (cycles per sample) centred at sample ``centre``."""
    a = (np.pi * freq * (np.arange(nt, dtype=np.float64) - centre)) ** 2
    return (1.0 - 2.0 * a) * np.exp(-a)


def ricker_traces(nt, ntrace, seed):
    """[nt, ntrace]: per trace the sum of three seeded Ricker wavelets (centres in the middle 60 % of the record, 0.02 to
    0.06 cycles per sample, amplitudes 0.5 to 1.5 of either sign) plus white noise of 1e-3 of the array's largest sample,
    rounded to float32 and returned as float64."""
    rng = np.random.default_rng(seed)
    x = np.zeros((nt, ntrace))
    for tr in range(ntrace):
        for _ in range(3):
            amp = rng.uniform(0.5, 1.5) * rng.choice([-1.0, 1.0])
            x[:, tr] += amp * ricker(nt, rng.uniform(0.2, 0.8) * nt, rng.uniform(0.02, 0.06))
    x += 1e-3 * np.abs(x).max() * rng.standard_normal(x.shape)
    return x.astype(np.float32).astype(np.float64)


SHIFTS = list(range(0, 61, 3))


def shifted_pair(shift):
    """The cycle-skipping pin, a one-trace record of 512 samples: a Ricker wavelet of 0.03 cycles per sample centred at
    256 (observed) and its copy ``shift`` samples later (modelled); 60 samples are almost two periods.  [512, 1] each."""
    return ricker(512, 256 + shift, 0.03)[:, None], ricker(512, 256, 0.03)[:, None]


def stage_and_window(a, sos, sel_dense):
    """W F a: F = scipy.signal.sosfilt along time (``sos`` None: identity), W the dense weights of a TraceSelection (None:
    identity).  W selects: a trace whose weights are all 0 is not read (it may hold NaN) and gives zeros."""
    from scipy import signal
    a = np.asarray(a, dtype=np.float64)
    if sel_dense is not None:
        a = np.where(sel_dense.any(axis=0), a, 0.0)
    if sos is not None:
        a = signal.sosfilt(sos, a, axis=0)
    return a if sel_dense is None else a * sel_dense


def composed(s, o, sos, sel_dense, eps=None, eps_rel=1e-3):
    """Loss and dloss/ds of envelope(W F s, W F o) (:func:`stage_and_window`); eps None: eps_rel * max|W F o|.
    Returns (loss, grad, eps)."""
    from scipy import signal
    ws, wo = stage_and_window(s, sos, sel_dense), stage_and_window(o, sos, sel_dense)
    if eps is None:
        eps = eps_rel * float(np.abs(wo).max())
    loss, adj = loss_adj(ws, wo, eps)
    if sel_dense is not None:
        adj = adj * sel_dense
    if sos is not None:
        adj = signal.sosfilt(sos, adj[::-1], axis=0)[::-1]
    return loss, adj, eps
