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


def l2_half(pred, obs, sos=None):
    """0.5 * sum((pred - obs)**2); with ``sos`` (:func:`butterworth_sos`) of the stage-filtered traces,
    0.5 * sum(F(pred - obs)**2), time on axis 0."""
    if sos is not None:
        return _FilteredMisfitFn.apply(pred, obs, _sos_array(sos), _lib.MISFIT_L2)
    return _MisfitFn.apply(pred, obs, None, _lib.MISFIT_L2)


def global_correlation(pred, obs, sos=None):
    """-sum over traces of <pred, obs> / (|pred| |obs|), time on axis 0 (insensitive to trace amplitudes); with ``sos``
    (:func:`butterworth_sos`) of the stage-filtered traces F pred, F obs."""
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
