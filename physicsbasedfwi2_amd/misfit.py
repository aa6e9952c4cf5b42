"""Fused data misfit + adjoint source on the GPU (csrc/mifwi_misfit.hip through the C-ABI).

Drop-in for the torch expressions the reference evaluates between the propagator call and
``.backward()``:

* ``l1_trace_normalized(pred, obs_norm, direct)``  -- models/networks.py:5467-5476, 5491
  (``obs_norm`` is the observed data already normalised per trace, networks.py:5418-5419)
* ``l2_half(pred, obs)`` -- ``0.5 * sum((pred - obs)**2)``, seisgan/fwi/layers.py:176-178 and
  DENISE's lnorm = 2 objective (networks.py:7758)

* ``global_correlation(pred, obs)`` -- ``-sum_traces <pred, obs> / (|pred| |obs|)``, DENISE's global-correlation
  norm (the ``lnorm`` argument of ``add_fwi_stage``, models/networks.py:9863, 10503)

* ``l2_half(pred, obs, sos)`` / ``global_correlation(pred, obs, sos)`` -- the same objectives of the traces filtered
  along time with the causal recursive Butterworth filter of a frequency stage (``add_fwi_stage(fc_low=, fc_high=)``,
  models/networks.py:6374 ... 11676; ``sos = butterworth_sos(dt, fc_low, fc_high, order)``), in one launch that also
  delivers the adjoint source through the transposed filter; ``trace_filter(x, sos)`` is the filter alone

* ``l2_half(pred, obs, sos, select=sel)`` / ``global_correlation(pred, obs, sos, select=sel)`` -- the same, with dead
  traces, trace weights and time windows (:class:`TraceSelection`, DENISE's TRKILL and TIMEWIN) taken out of the
  objective inside the same launch: W after the stage filter, before the norm; ``trace_window(x, sel)`` is W alone

* ``envelope(pred, obs, sos=None, select=None, eps=None)`` -- ``0.5 * sum((E(pred) - E(obs))**2)`` with the regularised
  envelope ``E(x) = sqrt(x**2 + H(x)**2 + eps**2)``, DENISE's lnorm = 6 (Chi, Dong and Liu 2014), for the first
  low-frequency stages: it does not cycle-skip where the three objectives above do.  H is the Hilbert transform through a
  DFT zero-padded to a power of two, an FFT held in LDS (csrc/mifwi_envelope.hip); one launch delivers the loss and the
  exact adjoint source.  With ``sos`` / ``select`` it is composed with ``trace_filter`` / ``trace_window``;
  ``trace_hilbert(x)`` is H alone (its backward is H^T = -H), ``trace_envelope(x, eps)`` the envelope as a torch expression

* ``transport(pred, obs, sos=None, select=None, b=None, b_rel=4.0)`` -- ``0.5 * sum over traces of W2**2``, the quadratic
  Wasserstein distance along time between the traces made positive by ``softplus(b x)`` and normalised to unit mass
  (Engquist and Froese 2014; Yang et al. 2018): it keeps growing with a time shift where even the envelope flattens.  The
  distribution functions live in LDS in double (csrc/mifwi_transport.hip); one launch delivers the loss and the exact
  adjoint source.  With ``sos`` / ``select`` it is composed with ``trace_filter`` / ``trace_window`` as ``envelope`` is

All return a 0-d tensor that back-propagates into ``pred`` (one kernel pass produces the loss and
dloss/dpred).  No CPU fallback: CPU tensors raise.

* ``estimate_matching_filter(pred, obs, lag_before, lag_after)`` and ``trace_convolve(x, h, lag_before)`` -- source-wavelet
  estimation (DENISE's INV_STF) in front of any of the objectives above: per shot, the finite-lag Wiener filter ``h`` with a
  water level that best maps the modelled traces onto the observed ones (``stf_correlations`` on the device,
  ``solve_matching_filter`` on the host in float64), and the convolution of traces ``[nt, nshot, nrec]`` with it, whose
  backward is its exact transpose (csrc/mifwi_stf.hip).  ``l2_half(trace_convolve(pred, h, lag_before), obs, ...)`` is the
  objective with the wavelet corrected; its gradient is exact with ``h`` held fixed.  This is this library's time-domain
  choice (libstfinv works in the frequency domain); the default water level 1e-2 is ours.
"""
import ctypes

import numpy as np
import torch

from . import _lib


class _MisfitFn(torch.autograd.Function):
    """Loss and adjoint source of ``kind`` in one call: mifwi_misfit_selected with ``select``, mifwi_misfit_filtered with
    ``sos`` alone, mifwi_misfit with neither (the only one that takes ``direct``)."""

    @staticmethod
    def forward(ctx, pred, obs, direct, sos, select, kind):
        if not pred.is_cuda:
            raise _lib.MifwiError("misfit needs CUDA/HIP tensors (libmifwi has no CPU fallback)")
        if pred.dim() < 2 or obs.shape != pred.shape or (direct is not None and direct.shape != pred.shape):
            raise ValueError("pred%s must share one [nt, ...] shape" % (", obs (and direct)" if sos is None and select is None
                                                                         else " and obs"))
        sel = None if select is None else select._on(pred.device, pred.shape[1:])
        lib = _lib.load()
        p = pred.detach().contiguous().float()
        o = obs.detach().contiguous().float()
        d = None if direct is None else direct.detach().contiguous().float()
        nt = p.shape[0]
        ntrace = p.numel() // nt
        adj = torch.empty_like(p) if pred.requires_grad else None
        loss = torch.empty((), device=p.device, dtype=torch.float32)
        head = (p.device.index or 0, kind, _lib.ptr(p), _lib.ptr(o))
        stage = (None, 0) if sos is None else (_sos_ptr(sos), sos.shape[0])
        if select is not None:
            elems = lib.mifwi_misfit_selected_work_elems(kind, nt, ntrace, stage[1])
            call, args = lib.mifwi_misfit_selected, head + (nt, ntrace) + stage + tuple(map(_lib.ptr, sel)) + (select.gamma,)
        elif sos is not None:
            elems = lib.mifwi_misfit_filtered_work_elems(kind, nt, ntrace)
            call, args = lib.mifwi_misfit_filtered, head + (nt, ntrace) + stage
        else:
            elems = lib.mifwi_misfit_work_elems(kind, nt, ntrace)
            call, args = lib.mifwi_misfit, head + (_lib.ptr(d), nt, ntrace)
        work = torch.empty(elems, device=p.device, dtype=torch.float32)
        _lib.check(call(*args, _lib.ptr(loss), _lib.ptr(adj), _lib.ptr(work), torch.cuda.current_stream(p.device).cuda_stream))
        ctx.adj = adj
        return loss

    @staticmethod
    def backward(ctx, g):
        # the adjoint source stays with the graph (a second backward through a retained graph gets it again)
        return (None if ctx.adj is None else ctx.adj * g), None, None, None, None, None


def l1_trace_normalized(pred, obs_norm, direct=None):
    """mean |(pred - direct) / (max_t |pred - direct| + 1e-10) - obs_norm|, time on axis 0."""
    return _MisfitFn.apply(pred, obs_norm, direct, None, None, _lib.MISFIT_L1_TRACE_NORM)


def l2_half(pred, obs, sos=None, select=None):
    """0.5 * sum((pred - obs)**2); with ``sos`` (:func:`butterworth_sos`) of the stage-filtered traces,
    0.5 * sum(F(pred - obs)**2), time on axis 0; with ``select`` (:class:`TraceSelection`) 0.5 * sum((W F(pred - obs))**2)."""
    return _MisfitFn.apply(pred, obs, None, None if sos is None else _sos_array(sos), select, _lib.MISFIT_L2)


def global_correlation(pred, obs, sos=None, select=None):
    """-sum over traces of <pred, obs> / (|pred| |obs|), time on axis 0 (insensitive to trace amplitudes); with ``sos``
    (:func:`butterworth_sos`) of the stage-filtered traces F pred, F obs; with ``select`` (:class:`TraceSelection`) of
    W F pred, W F obs."""
    return _MisfitFn.apply(pred, obs, None, None if sos is None else _sos_array(sos), select, _lib.MISFIT_GLOBAL_CORRELATION)


def butterworth_sos(dt, fc_low=0.0, fc_high=0.0, order=6):
    """Second-order sections of the stage filter of ``add_fwi_stage(fc_low, fc_high, order)`` at the time step ``dt``:
    float64 [nsec, 6] in scipy's row order b0 b1 b2 a0 a1 a2, or None when nothing is to be filtered.  The design of
    ``compat.pyapi_denise.butterworth``: ``scipy.signal.butter(order, fc / fnyq, ..., output="sos")``, the low-pass
    (corner fc_high) sections first, then the high-pass (corner fc_low); a corner <= 0 is absent, a low-pass corner at or
    above Nyquist is dropped.  More than MIFWI_FILTER_MAX_SECTIONS sections: ValueError."""
    from scipy import signal
    lo = float(fc_low) if fc_low and fc_low > 0 else 0.0
    hi = float(fc_high) if fc_high and fc_high > 0 else 0.0
    fnyq = 0.5 / dt
    if hi >= fnyq:
        hi = 0.0                                   # nothing to cut below Nyquist
    parts = []
    if hi > 0:
        parts.append(signal.butter(order, hi / fnyq, "lowpass", output="sos"))
    if lo > 0:
        parts.append(signal.butter(order, lo / fnyq, "highpass", output="sos"))
    if not parts:
        return None
    sos = np.ascontiguousarray(np.concatenate(parts, axis=0), dtype=np.float64)
    if sos.shape[0] > _lib.FILTER_MAX_SECTIONS:
        raise ValueError("order %d with corners (%g, %g) Hz makes %d second-order sections; the kernels take %d"
                         % (order, lo, hi, sos.shape[0], _lib.FILTER_MAX_SECTIONS))
    return sos


def _sos_array(sos):
    a = np.ascontiguousarray(sos, dtype=np.float64)
    if a.ndim != 2 or a.shape[1] != 6:
        raise ValueError("sos must be [nsec, 6] (b0 b1 b2 a0 a1 a2 per section)")
    return a


def _sos_ptr(sos):
    return sos.ctypes.data_as(ctypes.c_void_p)


class _TraceFilterFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, sos, transpose):
        if not x.is_cuda:
            raise _lib.MifwiError("trace_filter needs CUDA/HIP tensors (libmifwi has no CPU fallback)")
        if x.dim() < 1:
            raise ValueError("x must be [nt, ...]")
        lib = _lib.load()
        xc = x.detach().contiguous().float()
        y = torch.empty_like(xc)
        nt = xc.shape[0]
        if xc.numel():
            _lib.check(lib.mifwi_trace_filter(xc.device.index or 0, _lib.ptr(xc), _lib.ptr(y), nt, xc.numel() // nt,
                                              _sos_ptr(sos), sos.shape[0], int(transpose),
                                              torch.cuda.current_stream(xc.device).cuda_stream))
        ctx.sos, ctx.transpose = sos, transpose
        return y

    @staticmethod
    def backward(ctx, g):
        return _TraceFilterFn.apply(g, ctx.sos, not ctx.transpose), None, None


def trace_filter(x, sos, transpose=False):
    """y = F x along axis 0 (any trailing shape), F the cascade ``sos`` run as scipy.signal.sosfilt runs it (double state,
    zero initial conditions); ``transpose=True``: y = F^T x, the same recurrence from the last sample to the first.
    Differentiable: the backward of one is the other."""
    return _TraceFilterFn.apply(x, _sos_array(sos), bool(transpose))


class TraceSelection:
    """Which samples enter the objective: the diagonal operator W with

        w[t, tr] = weight[tr] * g(t),   d = max(t_on[tr] - t, t - t_off[tr], 0),   g = 1 where d == 0, else exp(-gamma d**2)

    ``t`` the sample index.  ``weight`` >= 0 (0 kills the trace; None: 1), ``t_on`` / ``t_off`` in samples (both or
    neither; they may lie outside the trace and may be reversed, which leaves no sample inside; None: no window),
    ``gamma`` >= 0 per sample**2 (``inf``: a boxcar).  The arrays have the trace shape ``pred.shape[1:]``; they are checked
    once here (finite, weight >= 0), kept as float32 and copied to a device the first time they are used there.
    W selects: a sample with w == 0 is not read into the sums, so a killed trace may hold NaN (csrc/mifwi_misfit_select.h)."""

    def __init__(self, weight=None, t_on=None, t_off=None, gamma=0.0):
        if (t_on is None) != (t_off is None):
            raise ValueError("a time window needs both t_on and t_off")
        self.gamma = float(gamma)
        if not self.gamma >= 0.0:
            raise ValueError("gamma=%r: the taper needs gamma >= 0 (inf: boxcar)" % (gamma,))
        self.weight, self.t_on, self.t_off = (None if a is None else self._array(a, n)
                                              for a, n in ((weight, "weight"), (t_on, "t_on"), (t_off, "t_off")))
        shapes = {a.shape for a in (self.weight, self.t_on, self.t_off) if a is not None}
        if len(shapes) > 1:
            raise ValueError("weight, t_on and t_off must share the trace shape, got %s" % sorted(shapes))
        self.shape = shapes.pop() if shapes else None          # None: nothing selected, any trace shape
        if self.weight is not None and not (self.weight >= 0).all():
            raise ValueError("trace weights must be >= 0 (0 kills a trace)")
        self._dev = {}

    @staticmethod
    def _array(a, name):
        a = np.ascontiguousarray(a.detach().cpu().numpy() if torch.is_tensor(a) else a, dtype=np.float32)
        if not np.isfinite(a).all():
            raise ValueError("%s must be finite" % name)
        return a

    @classmethod
    def from_kill(cls, kill):
        """``kill``: array of the trace shape, nonzero = the trace is dead."""
        kill = kill.detach().cpu().numpy() if torch.is_tensor(kill) else np.asarray(kill)
        return cls(weight=np.where(kill != 0, 0.0, 1.0))

    @classmethod
    def from_picks(cls, picks_s, before_s, after_s, dt, gamma_per_s2=float("inf"), weight=None):
        """The window [pick - before_s, pick + after_s] around picked times, all in seconds (arrays of the trace shape or
        scalars), at the time step ``dt``; ``gamma_per_s2``: the taper outside, exp(-gamma (distance in s)**2)."""
        picks = np.asarray(picks_s.detach().cpu().numpy() if torch.is_tensor(picks_s) else picks_s, dtype=np.float64)
        return cls(weight=weight, t_on=(picks - np.asarray(before_s, dtype=np.float64)) / dt,
                   t_off=(picks + np.asarray(after_s, dtype=np.float64)) / dt, gamma=float(gamma_per_s2) * dt * dt)

    def dense(self, nt):
        """The weights as float64 [nt, *trace shape]: the definition the kernels are tested against."""
        if self.shape is None:
            raise ValueError("a selection without arrays has no shape of its own")
        w = np.ones((nt,) + self.shape)
        if self.t_on is not None:
            t = np.arange(nt, dtype=np.float64).reshape((nt,) + (1,) * len(self.shape))
            d = np.maximum(np.maximum(self.t_on.astype(np.float64) - t, t - self.t_off.astype(np.float64)), 0.0)
            with np.errstate(invalid="ignore"):                  # inf * 0 where d == 0, replaced below
                w = np.where(d > 0, np.exp(-self.gamma * d * d), 1.0)
        if self.weight is not None:
            w = w * self.weight.astype(np.float64)
        return w

    def shots(self, sl):
        """The selection of the shots ``sl`` (a slice of the leading trace axis), for chunked or distributed use."""
        if not isinstance(sl, slice):
            raise ValueError("shots() takes a slice of the shot axis")
        if self.shape is not None and len(self.shape) < 2:
            raise ValueError("shots() needs a trace shape [nshot, nrec], this selection has %s" % (self.shape,))
        cut = lambda a: None if a is None else a[sl]
        return TraceSelection(cut(self.weight), cut(self.t_on), cut(self.t_off), self.gamma)

    def _on(self, device, shape):
        """(weight, t_on, t_off) on ``device`` (None where absent) for traces of ``shape``"""
        if self.shape is not None and tuple(shape) != self.shape:
            raise ValueError("the selection is for traces of shape %s, the data have %s" % (self.shape, tuple(shape)))
        if device not in self._dev:
            self._dev[device] = tuple(None if a is None else torch.from_numpy(a).to(device)
                                      for a in (self.weight, self.t_on, self.t_off))
        return self._dev[device]


class _TraceWindowFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, select):
        if not x.is_cuda:
            raise _lib.MifwiError("trace_window needs CUDA/HIP tensors (libmifwi has no CPU fallback)")
        if x.dim() < 2:
            raise ValueError("x must be [nt, ...]")
        a, on, off = select._on(x.device, x.shape[1:])
        lib = _lib.load()
        xc = x.detach().contiguous().float()
        y = torch.empty_like(xc)
        nt = xc.shape[0]
        if xc.numel():
            _lib.check(lib.mifwi_trace_window(xc.device.index or 0, _lib.ptr(xc), _lib.ptr(y), nt, xc.numel() // nt,
                                              _lib.ptr(a), _lib.ptr(on), _lib.ptr(off), select.gamma,
                                              torch.cuda.current_stream(xc.device).cuda_stream))
        ctx.select = select
        return y

    @staticmethod
    def backward(ctx, g):
        return _TraceWindowFn.apply(g, ctx.select), None


def trace_window(x, select):
    """y = W x, W the diagonal of ``select`` (:class:`TraceSelection`), time on axis 0.  Differentiable: W is its own
    transpose, so the backward is the same call."""
    return _TraceWindowFn.apply(x, select)


# ---- envelope objective: Hilbert transform, envelope residual and its adjoint (csrc/mifwi_envelope.hip) ----------------
class _TraceHilbertFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, transpose):
        if not x.is_cuda:
            raise _lib.MifwiError("trace_hilbert needs CUDA/HIP tensors (libmifwi has no CPU fallback)")
        if x.dim() < 1:
            raise ValueError("x must be [nt, ...]")
        lib = _lib.load()
        xc = x.detach().contiguous().float()
        y = torch.empty_like(xc)
        nt = xc.shape[0]
        if xc.numel():
            _lib.check(lib.mifwi_trace_hilbert(xc.device.index or 0, _lib.ptr(xc), _lib.ptr(y), nt, xc.numel() // nt,
                                               int(transpose), torch.cuda.current_stream(xc.device).cuda_stream))
        ctx.transpose = transpose
        return y

    @staticmethod
    def backward(ctx, g):
        return _TraceHilbertFn.apply(g, not ctx.transpose), None


def trace_hilbert(x, transpose=False):
    """y = H x along axis 0 (any trailing shape): the Hilbert transform through a DFT zero-padded to N, the smallest power
    of two >= nt, ``scipy.signal.hilbert(x, N=N, axis=0).imag[:nt]``; nt <= 8192.  ``transpose=True``: y = H^T x = -H x, the
    negated bits.  Differentiable: the backward of one is the other."""
    return _TraceHilbertFn.apply(x, bool(transpose))


def trace_envelope(x, eps):
    """E(x) = sqrt(x**2 + H(x)**2 + eps**2) along axis 0 as a torch expression over :func:`trace_hilbert`: differentiable
    through autograd, for quality control and as a cross-check of :func:`envelope`.  ``eps`` > 0 keeps the square root
    differentiable where the trace is silent."""
    h = trace_hilbert(x)
    return torch.sqrt(x * x + h * h + float(eps) ** 2)


class _EnvelopeFn(torch.autograd.Function):
    """Loss and adjoint source of the envelope objective in one call of mifwi_misfit_envelope."""

    @staticmethod
    def forward(ctx, pred, obs, eps):
        if not pred.is_cuda:
            raise _lib.MifwiError("misfit needs CUDA/HIP tensors (libmifwi has no CPU fallback)")
        if pred.dim() < 2 or obs.shape != pred.shape:
            raise ValueError("pred and obs must share one [nt, ...] shape")
        lib = _lib.load()
        p = pred.detach().contiguous().float()
        o = obs.detach().contiguous().float()
        nt = p.shape[0]
        ntrace = p.numel() // nt
        adj = torch.empty_like(p) if pred.requires_grad else None
        loss = torch.empty((), device=p.device, dtype=torch.float32)
        work = torch.empty(max(int(lib.mifwi_misfit_envelope_work_elems(nt, ntrace)), 2), device=p.device, dtype=torch.float32)
        _lib.check(lib.mifwi_misfit_envelope(p.device.index or 0, _lib.ptr(p), _lib.ptr(o), nt, ntrace, float(eps), _lib.ptr(loss),
                                             _lib.ptr(adj), _lib.ptr(work), torch.cuda.current_stream(p.device).cuda_stream))
        ctx.adj = adj
        return loss

    @staticmethod
    def backward(ctx, g):
        # as _MisfitFn: the adjoint source stays with the graph
        return (None if ctx.adj is None else ctx.adj * g), None, None


def envelope(pred, obs, sos=None, select=None, eps=None, eps_rel=1e-3):
    """0.5 * sum((E(pred) - E(obs))**2), E(x) = sqrt(x**2 + H(x)**2 + eps**2) the regularised envelope, time on axis 0
    (Chi, Dong and Liu 2014; DENISE's lnorm = 6): one launch for the Hilbert transforms, the residual and the exact adjoint
    source ``r pred / E - H(r H(pred) / E)``, r the envelope residual.  It does not cycle-skip where the sample-by-sample
    objectives do.  nt <= 8192; H as in :func:`trace_hilbert`.

    With ``sos`` (:func:`butterworth_sos`) and / or ``select`` (:class:`TraceSelection`) it is the composition
    ``envelope(W F pred, W F obs)`` through :func:`trace_filter` and :func:`trace_window` (``obs`` is detached); autograd
    carries the adjoint source back through W and F^T.

    ``eps`` is one absolute scalar >= 0.  ``eps=None``: ``eps_rel * max|W F obs|``, a constant of the data, so the gradient
    stays exact; all-zero data give eps = 0, where a sample with E(pred) == 0 contributes nothing to the adjoint source.
    Ranks of ``dist.py`` that each hold some of the shots should pass one explicit ``eps``: otherwise every rank derives its
    own from the shots it holds."""
    obs = obs.detach()
    if sos is not None:
        sos = _sos_array(sos)
        pred, obs = trace_filter(pred, sos), trace_filter(obs, sos)
    if select is not None:
        pred, obs = trace_window(pred, select), trace_window(obs, select)
    if eps is None:
        eps = float(eps_rel) * float(obs.abs().max()) if obs.numel() else 0.0
    return _EnvelopeFn.apply(pred, obs, float(eps))


# ---- optimal-transport objective: W2 between normalised traces and its adjoint source (csrc/mifwi_transport.hip) --------
class _TransportFn(torch.autograd.Function):
    """Loss and adjoint source of the transport objective in one call of mifwi_misfit_transport."""

    @staticmethod
    def forward(ctx, pred, obs, b):
        if not pred.is_cuda:
            raise _lib.MifwiError("misfit needs CUDA/HIP tensors (libmifwi has no CPU fallback)")
        if pred.dim() < 2 or obs.shape != pred.shape:
            raise ValueError("pred and obs must share one [nt, ...] shape")
        lib = _lib.load()
        p = pred.detach().contiguous().float()
        o = obs.detach().contiguous().float()
        nt = p.shape[0]
        ntrace = p.numel() // nt
        adj = torch.empty_like(p) if pred.requires_grad else None
        loss = torch.empty((), device=p.device, dtype=torch.float32)
        work = torch.empty(max(int(lib.mifwi_misfit_transport_work_elems(nt, ntrace)), 2), device=p.device, dtype=torch.float32)
        _lib.check(lib.mifwi_misfit_transport(p.device.index or 0, _lib.ptr(p), _lib.ptr(o), nt, ntrace, float(b), _lib.ptr(loss),
                                              _lib.ptr(adj), _lib.ptr(work), torch.cuda.current_stream(p.device).cuda_stream))
        ctx.adj = adj
        return loss

    @staticmethod
    def backward(ctx, g):
        # as _MisfitFn: the adjoint source stays with the graph
        return (None if ctx.adj is None else ctx.adj * g), None, None


def transport(pred, obs, sos=None, select=None, b=None, b_rel=4.0):
    """0.5 * sum over traces of W2(p, q)**2 along time (axis 0, in samples): the quadratic Wasserstein distance between the
    traces made positive by ``softplus(b x)`` and normalised to unit mass (Engquist and Froese 2014; Yang et al. 2018), every
    trace on its own.  With P, Q the running sums of p, q and T the inverse of the piecewise-linear Q at the cell midpoints
    of P, ``W = sum_k p_k (k + 1/2 - T_k)**2``; one launch delivers the loss and its exact adjoint source (the definition in
    full: include/mifwi.h, "TRANSPORT MISFIT").  It compares where the energy sits in time and keeps growing with a time shift
    where :func:`l2_half` cycle-skips.  nt <= 8192.  ``pred`` with the bits of ``obs`` gives exact zeros.

    With ``sos`` (:func:`butterworth_sos`) and / or ``select`` (:class:`TraceSelection`) it is the composition
    ``transport(W F pred, W F obs)`` through :func:`trace_filter` and :func:`trace_window`, as :func:`envelope` composes them
    (``obs`` is detached); a killed trace is a pair of zero traces there and costs nothing.

    ``b`` is one absolute scalar > 0.  ``b=None``: ``b_rel / max|W F obs|``, a constant of the data, so the gradient stays
    exact; all-zero observed data then raise ``MifwiError``.  At ``b_rel`` 1 and 2 the loss of a shifted Ricker wavelet does
    not grow strictly with the shift, at 4 it does: that is the default.  Ranks of ``dist.py`` that each hold some of the
    shots should pass one explicit ``b``: otherwise every rank derives its own from the shots it holds."""
    obs = obs.detach()
    if sos is not None:
        sos = _sos_array(sos)
        pred, obs = trace_filter(pred, sos), trace_filter(obs, sos)
    if select is not None:
        pred, obs = trace_window(pred, select), trace_window(obs, select)
    if b is None:
        peak = float(obs.abs().max()) if obs.numel() else 0.0
        if not peak > 0.0:
            raise _lib.MifwiError("transport: the observed data are all zero (or not finite), so b = b_rel / max|obs| does not "
                                  "exist; pass b")
        b = float(b_rel) / peak
    return _TransportFn.apply(pred, obs, float(b))


# ---- matching filter: source-wavelet estimation in front of the objective (csrc/mifwi_stf.hip) -------------------------
def _lags(lag_before, lag_after):
    lb, la = int(lag_before), int(lag_after)
    if lb < 0 or la < 0 or lb + la + 1 > _lib.STF_MAX_LAGS:
        raise ValueError("lags before=%d after=%d: both >= 0 and before + after + 1 <= %d" % (lb, la, _lib.STF_MAX_LAGS))
    return lb, la


def stf_correlations(pred, obs, lag_before, lag_after, select=None):
    """The correlations behind the matching filter of traces ``[nt, nshot, nrec]``, per shot, summed in double:

        a[s, j] = sum_r w**2 sum_t pred[t] pred[t + j]           j = 0 .. nlag - 1,  nlag = lag_before + lag_after + 1
        c[s, i] = sum_r w**2 sum_t obs[t] pred[t - (i - lag_before)]

    (terms outside the record are absent).  ``select``: a :class:`TraceSelection` with a ``weight`` only - w multiplies the
    traces, a trace with w == 0 is not read; window the traces with :func:`trace_window` first if windows are wanted.
    Returns float64 device tensors ``[nshot, nlag]``.  Fixed summation order: identical calls give identical bits."""
    if not pred.is_cuda:
        raise _lib.MifwiError("stf_correlations needs CUDA/HIP tensors (libmifwi has no CPU fallback)")
    if pred.dim() != 3 or obs.shape != pred.shape:
        raise ValueError("pred and obs must share one [nt, nshot, nrec] shape")
    lb, la = _lags(lag_before, lag_after)
    w = None
    if select is not None:
        if select.t_on is not None:
            raise ValueError("stf_correlations takes trace weights only: apply the time windows to both sides with "
                             "trace_window(x, select) first and pass a selection that holds the weight alone")
        w = select._on(pred.device, pred.shape[1:])[0]
    lib = _lib.load()
    p = pred.detach().contiguous().float()
    o = obs.detach().contiguous().float()
    nt, ns, nr = p.shape
    a = torch.empty((ns, lb + la + 1), device=p.device, dtype=torch.float64)
    c = torch.empty_like(a)
    if p.numel() == 0:
        raise ValueError("empty traces")
    work = torch.empty(lib.mifwi_stf_correlate_work_elems(nt, ns, nr, lb, la), device=p.device, dtype=torch.float32)
    _lib.check(lib.mifwi_stf_correlate(p.device.index or 0, _lib.ptr(p), _lib.ptr(o), _lib.ptr(w), nt, ns, nr, lb, la,
                                       _lib.ptr(a), _lib.ptr(c), _lib.ptr(work),
                                       torch.cuda.current_stream(p.device).cuda_stream))
    return a, c


def solve_matching_filter(a, c, water_level=1e-2, per_shot=True, lag_before=0):
    """The filter of the correlations ``a``, ``c`` ``[nshot, nlag]`` (:func:`stf_correlations`; CPU or device tensors):
    per shot ``T h = c`` with ``T[i, j] = a[|i - j|] + water_level * a[0] * (i == j)``, solved in float64 on the host.
    ``water_level`` > 0 (1e-2 is this library's default).  A shot without energy (``a[0] == 0``) gets the unit spike at lag
    0, which sits at index ``lag_before``.  ``per_shot=False``: the correlations are summed over the shots first and every
    shot gets the one filter.  Returns float64 CPU ``[nshot, nlag]``.

    The autocorrelation (Toeplitz) method: ``h`` is the exact least-squares filter only when the modelled traces have died
    out ``lag_after`` samples before the record ends and start ``lag_before`` samples after it begins."""
    if not float(water_level) > 0:
        raise ValueError("water_level=%r: the water level must be > 0" % (water_level,))
    a = torch.as_tensor(a).detach().to("cpu", torch.float64)
    c = torch.as_tensor(c).detach().to("cpu", torch.float64)
    if a.dim() != 2 or a.shape != c.shape:
        raise ValueError("a and c must share one [nshot, nlag] shape")
    ns, nlag = a.shape
    if not 0 <= int(lag_before) < nlag:
        raise ValueError("lag_before=%r is not a lag of a filter with %d taps" % (lag_before, nlag))
    if not per_shot:
        a, c = a.sum(0, keepdim=True), c.sum(0, keepdim=True)
    idx = (torch.arange(nlag)[:, None] - torch.arange(nlag)[None, :]).abs()
    h = torch.zeros_like(c)
    for s in range(a.shape[0]):
        if a[s, 0] == 0:
            h[s, int(lag_before)] = 1.0
            continue
        t = a[s][idx] + float(water_level) * a[s, 0] * torch.eye(nlag, dtype=torch.float64)
        h[s] = torch.linalg.solve(t, c[s])
    return h if per_shot else h.expand(ns, nlag).contiguous()


class _TraceConvolveFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, h, lag_before, transpose):
        if not x.is_cuda:
            raise _lib.MifwiError("trace_convolve needs CUDA/HIP tensors (libmifwi has no CPU fallback)")
        if x.dim() != 3 or h.dim() != 2 or h.shape[0] != x.shape[1]:
            raise ValueError("x must be [nt, nshot, nrec] and h [nshot, nlag]")
        lb, la = _lags(lag_before, h.shape[1] - 1 - int(lag_before))
        lib = _lib.load()
        xc = x.detach().contiguous().float()
        y = torch.empty_like(xc)
        nt, ns, nr = xc.shape
        if xc.numel():
            _lib.check(lib.mifwi_trace_convolve(xc.device.index or 0, _lib.ptr(xc), _lib.ptr(y), _lib.ptr(h), nt, ns, nr, lb, la,
                                                int(transpose), torch.cuda.current_stream(xc.device).cuda_stream))
        ctx.h, ctx.lag_before, ctx.transpose = h, lb, transpose
        return y

    @staticmethod
    def backward(ctx, g):
        return _TraceConvolveFn.apply(g, ctx.h, ctx.lag_before, not ctx.transpose), None, None, None


def trace_convolve(x, h, lag_before, transpose=False):
    """y[t, s, r] = sum_i h[s, i] x[t - (i - lag_before), s, r] for traces ``[nt, nshot, nrec]`` and per-shot taps
    ``h [nshot, nlag]`` (terms outside the record are absent); ``transpose=True``: the same sum with x[t + (i - lag_before)].
    Differentiable in ``x``: the backward of one is the other.  ``h`` is held fixed (no gradient)."""
    h = torch.as_tensor(h).detach().to(device=x.device, dtype=torch.float32).contiguous()
    return _TraceConvolveFn.apply(x, h, int(lag_before), bool(transpose))


def estimate_matching_filter(pred, obs, lag_before, lag_after, water_level=1e-2, sos=None, select=None, per_shot=True):
    """The matching filter of ``pred`` onto ``obs`` (:func:`stf_correlations`, :func:`solve_matching_filter`) as a float32
    device tensor ``[nshot, nlag]`` for :func:`trace_convolve`.  With ``sos`` it is estimated from the stage-filtered traces
    of both sides - the filter commutes with the stage, so it belongs in front of ``l2_half(..., sos=sos)`` unchanged.
    Nothing here is differentiated."""
    with torch.no_grad():
        if sos is not None:
            pred, obs = trace_filter(pred, sos), trace_filter(obs, sos)
        a, c = stf_correlations(pred, obs, lag_before, lag_after, select)
    h = solve_matching_filter(a, c, water_level, per_shot, lag_before)
    return h.to(device=pred.device, dtype=torch.float32)
