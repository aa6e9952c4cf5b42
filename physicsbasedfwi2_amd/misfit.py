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

All return a 0-d tensor that back-propagates into ``pred`` (one kernel pass produces the loss and
dloss/dpred).  No CPU fallback: CPU tensors raise.
"""
import ctypes

import numpy as np
import torch

from . import _lib


class _MisfitFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, obs, direct, kind):
        if not pred.is_cuda:
            raise _lib.MifwiError("misfit needs CUDA/HIP tensors (libmifwi has no CPU fallback)")
        if pred.dim() < 2 or obs.shape != pred.shape or (direct is not None and direct.shape != pred.shape):
            raise ValueError("pred, obs (and direct) must share one [nt, ...] shape")
        lib = _lib.load()
        p = pred.detach().contiguous().float()
        o = obs.detach().contiguous().float()
        d = None if direct is None else direct.detach().contiguous().float()
        nt = p.shape[0]
        ntrace = p.numel() // nt
        need_adj = pred.requires_grad
        adj = torch.empty_like(p) if need_adj else None
        loss = torch.empty((), device=p.device, dtype=torch.float32)
        work = torch.empty(lib.mifwi_misfit_work_elems(kind, nt, ntrace), device=p.device, dtype=torch.float32)
        _lib.check(lib.mifwi_misfit(p.device.index or 0, kind, _lib.ptr(p), _lib.ptr(o), _lib.ptr(d), nt,
                                    ntrace, _lib.ptr(loss), _lib.ptr(adj), _lib.ptr(work),
                                    torch.cuda.current_stream(p.device).cuda_stream))
        ctx.adj = adj
        return loss

    @staticmethod
    def backward(ctx, g):
        # the adjoint source stays with the graph (a second backward through a retained graph gets it again)
        return (None if ctx.adj is None else ctx.adj * g), None, None, None


def l1_trace_normalized(pred, obs_norm, direct=None):
    """mean |(pred - direct) / (max_t |pred - direct| + 1e-10) - obs_norm|, time on axis 0."""
    return _MisfitFn.apply(pred, obs_norm, direct, _lib.MISFIT_L1_TRACE_NORM)


def l2_half(pred, obs, sos=None, select=None):
    """0.5 * sum((pred - obs)**2); with ``sos`` (:func:`butterworth_sos`) of the stage-filtered traces,
    0.5 * sum(F(pred - obs)**2), time on axis 0; with ``select`` (:class:`TraceSelection`) 0.5 * sum((W F(pred - obs))**2)."""
    if select is not None:
        return _SelectedMisfitFn.apply(pred, obs, None if sos is None else _sos_array(sos), _lib.MISFIT_L2, select)
    if sos is not None:
        return _FilteredMisfitFn.apply(pred, obs, _sos_array(sos), _lib.MISFIT_L2)
    return _MisfitFn.apply(pred, obs, None, _lib.MISFIT_L2)


def global_correlation(pred, obs, sos=None, select=None):
    """-sum over traces of <pred, obs> / (|pred| |obs|), time on axis 0 (insensitive to trace amplitudes); with ``sos``
    (:func:`butterworth_sos`) of the stage-filtered traces F pred, F obs; with ``select`` (:class:`TraceSelection`) of
    W F pred, W F obs."""
    if select is not None:
        return _SelectedMisfitFn.apply(pred, obs, None if sos is None else _sos_array(sos), _lib.MISFIT_GLOBAL_CORRELATION,
                                       select)
    if sos is not None:
        return _FilteredMisfitFn.apply(pred, obs, _sos_array(sos), _lib.MISFIT_GLOBAL_CORRELATION)
    return _MisfitFn.apply(pred, obs, None, _lib.MISFIT_GLOBAL_CORRELATION)


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


class _FilteredMisfitFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, obs, sos, kind):
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
        work = torch.empty(lib.mifwi_misfit_filtered_work_elems(kind, nt, ntrace), device=p.device, dtype=torch.float32)
        _lib.check(lib.mifwi_misfit_filtered(p.device.index or 0, kind, _lib.ptr(p), _lib.ptr(o), nt, ntrace, _sos_ptr(sos),
                                             sos.shape[0], _lib.ptr(loss), _lib.ptr(adj), _lib.ptr(work),
                                             torch.cuda.current_stream(p.device).cuda_stream))
        ctx.adj = adj
        return loss

    @staticmethod
    def backward(ctx, g):
        return (None if ctx.adj is None else ctx.adj * g), None, None, None


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


class _SelectedMisfitFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, obs, sos, kind, select):
        if not pred.is_cuda:
            raise _lib.MifwiError("misfit needs CUDA/HIP tensors (libmifwi has no CPU fallback)")
        if pred.dim() < 2 or obs.shape != pred.shape:
            raise ValueError("pred and obs must share one [nt, ...] shape")
        a, on, off = select._on(pred.device, pred.shape[1:])
        lib = _lib.load()
        p = pred.detach().contiguous().float()
        o = obs.detach().contiguous().float()
        nt = p.shape[0]
        ntrace = p.numel() // nt
        nsec = 0 if sos is None else sos.shape[0]
        adj = torch.empty_like(p) if pred.requires_grad else None
        loss = torch.empty((), device=p.device, dtype=torch.float32)
        work = torch.empty(lib.mifwi_misfit_selected_work_elems(kind, nt, ntrace, nsec), device=p.device, dtype=torch.float32)
        _lib.check(lib.mifwi_misfit_selected(p.device.index or 0, kind, _lib.ptr(p), _lib.ptr(o), nt, ntrace,
                                             None if sos is None else _sos_ptr(sos), nsec, _lib.ptr(a), _lib.ptr(on),
                                             _lib.ptr(off), select.gamma, _lib.ptr(loss), _lib.ptr(adj), _lib.ptr(work),
                                             torch.cuda.current_stream(p.device).cuda_stream))
        ctx.adj = adj
        return loss

    @staticmethod
    def backward(ctx, g):
        return (None if ctx.adj is None else ctx.adj * g), None, None, None, None


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
