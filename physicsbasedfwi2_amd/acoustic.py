"""Host side of the acoustic propagator: plan handling, buffer allocation (torch = device
memory + stream plumbing only) and the ``torch.autograd.Function`` through which the model
gradient reaches the caller, as deepwave's autograd backward does at
models/networks.py:5464/5491 and ``FWILoss`` does at seisgan/fwi/layers.py:158-197.

All arithmetic happens in libmifwi.so (HIP); there is no CPU path here.
"""
import os

import torch

from . import _lib
from ._lib import MifwiError
from ._driver import (_GEOMETRIES, _Geometry, _MomentsHolder, _Plan, _require_cuda, _stream,  # noqa: F401 (re-exported)
                      Physics, Propagate, linearised, pad_columns)

# snapshots kept resident between forward and backward; above this the time axis is cut
# into checkpointed segments that are re-propagated during the adjoint (exact, ~1 extra forward)
DEFAULT_SNAPSHOT_BUDGET = 96 << 30


class AcousticPlan(_Plan):
    PREFIX, LAYOUT = "acoustic", _lib.AcousticLayout

    def __init__(self, n0, n1, nt, nshot, nsrc, nrec, ntap, c0, c1, device_index,
                 shots_per_group=0, edge_rows=0, cpml_width=0):
        self._create(_lib.AcousticDesc(n0, n1, nt, nshot, nsrc, nrec, ntap, c0, c1,
                                       shots_per_group, int(edge_rows), int(cpml_width)), device_index)


class PseudoHessian(_MomentsHolder):
    """Holder of the snapshot second moment behind the diagonal pseudo-Hessian of the scalar scheme (Shin's
    preconditioner; the counterpart of ``elastic.PseudoHessian``): pass it to :func:`propagate` (``pseudo_hessian=``)
    and every backward pass through that call adds ``M = sum (G^n)^2`` of its forward snapshot planes - summed over its
    shots and over the steps n < nt - 1 with ``n % stride == 0``, each weighted by ``stride`` - into ``.moments``
    [n0, n1] (None before the first backward).  The holder accumulates over calls (shot chunks, ranks' shares);
    :meth:`reset` zeroes it.  The pass is one more read of the snapshot buffer the backward holds
    (``mifwi_acoustic_snapshot_moments``), no extra propagation; ``stride = 4`` reads a quarter of it."""

    def _hessian(self, what, parametrization, model, pad, scale):
        mom = self._held(what)
        n0, n1 = mom.shape
        pad = int(pad)
        nz, nx = n0 - 2 * pad, n1 - 2 * pad
        mdl, = self._model_planes(what, mom, (model,), (nz, nx),
                                  "(moments [%d, %d], pad %d), got %%(got)s" % (n0, n1, pad), pad >= 0)
        out = torch.empty((nz, nx), device=mom.device, dtype=torch.float32)
        with torch.cuda.device(mom.device):
            _lib.check(_lib.load().mifwi_acoustic_pseudo_hessian(
                mom.device.index or 0, parametrization, _lib.ptr(mdl), _lib.ptr(mom), nz, nx, pad, n1, float(scale),
                _lib.ptr(out), _stream()))
        return out

    def hessian_velocity(self, vp, dt_over_h, pad):
        """[nz, nx]: the pseudo-Hessian of ``vp`` in the deepwave protocol, where ``r = (vp dt/h)^2`` with the model
        edge-replicated into a layer of ``pad`` cells: ``(2 vp (dt/h)^2)^2`` times the moments of the padded cells that
        replicate each model cell.  Finite and >= 0; 0 where vp = 0."""
        return self._hessian("hessian_velocity", _lib.AC_PARAM_VELOCITY, vp, pad, dt_over_h)

    def hessian_slowness2(self, m, s_over_h):
        """[n0, n1]: the pseudo-Hessian of the square slowness ``m = 1/vp^2`` on the padded grid (the seisgan
        protocol, every padded cell its own variable), ``r = (s/h)^2 / m``: ``(r/m)^2 M``.  0 where m <= 0."""
        return self._hessian("hessian_slowness2", _lib.AC_PARAM_SLOWNESS2, m, 0, s_over_h)

    @staticmethod
    def precondition(grad, hess, eps):
        """``grad / (hess / max(hess) + eps)`` on the device (``mifwi_gradient_precondition`` with one plane);
        grad, hess [nz, nx] tensors on a HIP device, eps > 0 the water level.  Returns a new tensor."""
        from . import conditioning
        if grad.dim() != 2:
            raise MifwiError("precondition: grad and hess must be [nz, nx] planes")
        return conditioning.precondition_gradients(grad[None], torch.as_tensor(hess)[None], eps)[0]


def _acoustic_inputs(r, q0, q1, cpml_width, gp):
    """r, q0, q1 as the C calls take them: float32 on r's device, the rows of r and q1 padded with 0 to gp columns."""
    n0, n1 = r.shape
    if cpml_width > 0 and (tuple(q0.shape) != (2, n0) or tuple(q1.shape) != (2, n1)):
        # q0 / q1 carry the layer's a, b profiles: [2, n0], [2, n1] -> [2, gp]
        raise MifwiError("cpml_width > 0: q0 / q1 must be the [2, n0] / [2, n1] C-PML profiles (a, b)")
    dev = r.device
    return (pad_columns(r, gp), q0.to(device=dev, dtype=torch.float32).contiguous(),
            pad_columns(q1.to(device=dev, dtype=torch.float32), gp))


def _forward_call(plan, coef, f_d, geo, rec):
    """``forward(snap_ptr, work_ptr, b, e, flags)`` as the drivers take it; ``rec`` = [traces], or None: a re-run that
    samples nothing."""
    lib = _lib.load()
    args = (plan.handle, *coef, _lib.ptr(f_d), *geo, _lib.ptr(rec[0] if rec else None))
    return lambda snap, work, b, e, flags: _lib.check(
        lib.mifwi_acoustic_forward(*args, snap, work, b, e, flags, _stream()))


def _adjoint_call(plan, coef, geo, g, grad_r, grad_f, work):
    """``adjoint(snap_ptr, snap_first, hi, lo, flags)`` as the backward driver takes it; g = [adjoint source]."""
    lib = _lib.load()
    return lambda snap, first, hi, lo, flags: _lib.check(lib.mifwi_acoustic_backward(
        plan.handle, *coef, *geo, _lib.ptr(g[0]), snap, first, _lib.ptr(grad_r), _lib.ptr(grad_f), _lib.ptr(work), hi, lo,
        flags, _stream()))


def _born_call(plan, coef, dr_p, df_d, geo, snap, drec, work, nt):
    _lib.check(_lib.load().mifwi_acoustic_born(plan.handle, *coef, _lib.ptr(dr_p), geo[2], geo[3], _lib.ptr(snap), 0,
                                               _lib.ptr(drec[0]), _lib.ptr(work), 0, nt, _lib.ZERO_STATE, _stream()))


class _Acoustic(Physics):
    """The scalar scheme as :class:`_driver.Propagate` and :func:`_driver.linearised` see it.  opts: c0, c1,
    shots_per_group, edge_rows, cpml_width."""
    name = rule = "acoustic"
    model = "r"
    zero_moments = True         # G^{nt-1} never reaches a recorded sample: no range ends the run, a run of one step has none
    not_served = "products across time checkpoints are not served"
    weight_returns = "a tensor of the shape of its argument"
    Plan = AcousticPlan
    forward_call, adjoint_call, born_call = (staticmethod(fn) for fn in (_forward_call, _adjoint_call, _born_call))
    inputs = staticmethod(lambda r, q0, q1, gp, o: _acoustic_inputs(r, q0, q1, o["cpml_width"], gp))
    snap_step = staticmethod(lambda lay, ns: (ns, lay.coef_elems // lay.gp, lay.gp))
    traces = staticmethod(lambda o: 1)
    weigh = staticmethod(lambda weight, drec: (weight(drec[0]),))


def _options(c0, c1, shots_per_group, edge_rows, cpml_width):
    return dict(c0=float(c0), c1=float(c1), shots_per_group=int(shots_per_group), edge_rows=int(edge_rows),
                cpml_width=int(cpml_width))


def propagate(r, f, q0, q1, src_cell, src_w, rec_cell, rec_w, c0=1.0, c1=1.0,
              shots_per_group=0, snapshot_budget=DEFAULT_SNAPSHOT_BUDGET, edge_rows=0, cpml_width=0, pseudo_hessian=None):
    """Run the acoustic propagator (differentiable w.r.t. ``r`` and ``f``).

    cpml_width = W > 0: the absorbing layer is a second-order convolutional PML of W cells on every side instead of
    the sponge; q0 [2, n0] and q1 [2, n1] then hold its a and b profiles (``profiles.cpml_tables(...)[:2]``), zero
    outside the layer.  Same call otherwise; runs on the one-launch-per-step kernels.

    r   [n0,n1]  = vp^2 dt^2 / h^2 on the computational (already padded) grid
    f   [nt,nshot,nsrc] source amplitudes (the injected term is  w * f[n] * r[cell])
    q0  [n0], q1 [n1]  separable damping,  q = damp h^2 / (2 dt)
    src_cell/src_w [nshot,nsrc,ntap], rec_cell/rec_w [nshot,nrec,ntap]  (cell = i0*n1+i1)
    edge_rows: optional hint, rows of absorbing layer at the top/bottom of the grid (performance only)
    pseudo_hessian: a :class:`PseudoHessian` holder, or None.  The backward pass through this call then adds the second
    moment of its snapshot planes G^0 .. G^{nt-2} into the holder (one more read of the snapshot buffer - resident, or
    every regenerated checkpoint segment once); a run that needs no gradient has no such pass and raises.  Without a
    holder nothing changes: the same launches, the same results.
    returns rec [nt,nshot,nrec] with rec[n] sampled from u^n.
    """
    if pseudo_hessian is not None and not isinstance(pseudo_hessian, PseudoHessian):
        raise MifwiError("pseudo_hessian must be an acoustic.PseudoHessian holder or None")
    _require_cuda(r, "r")
    geom = _Geometry.get(src_cell, src_w, rec_cell, rec_w, r.device)
    f = f.to(device=r.device)
    ntap = geom.src_cell.shape[2]
    if ntap > 1 and not cpml_width and _flatten_taps_pays(r, f, geom, c0, c1, edge_rows):
        # Bilinear taps (the Devito-shaped protocol) as independent single-cell points: every tap becomes
        # a source / receiver of its own, which makes the single-launch time loop eligible; the taps of a
        # point are recombined by differentiable torch ops (sum over the tap axis, repeat of f).
        ns, nsrc = geom.src_cell.shape[:2]
        nrec = geom.rec_cell.shape[1]
        flat = _Geometry(geom.src_cell.reshape(ns, nsrc * ntap, 1), geom.src_w.reshape(ns, nsrc * ntap, 1),
                         geom.rec_cell.reshape(ns, nrec * ntap, 1), geom.rec_w.reshape(ns, nrec * ntap, 1),
                         r.device)
        rec, = Propagate.apply(r, f.repeat_interleave(ntap, dim=2), _Acoustic, q0, q1, flat, int(snapshot_budget),
                               pseudo_hessian, _options(c0, c1, shots_per_group, edge_rows, 0))
        return rec.reshape(rec.shape[0], ns, nrec, ntap).sum(dim=3)
    return Propagate.apply(r, f, _Acoustic, q0, q1, geom, int(snapshot_budget), pseudo_hessian,
                           _options(c0, c1, shots_per_group, edge_rows, cpml_width))[0]


def _flatten_taps_pays(r, f, geom, c0, c1, edge_rows):
    """True when the flattened (single-tap) problem runs on the single-launch kernels' fast paths."""
    if os.environ.get("MIFWI_AC_FLATTEN_TAPS", "1") == "0":
        return False
    ns, nsrc, ntap = geom.src_cell.shape
    nrec = geom.rec_cell.shape[1]
    if nrec * ntap > 1024 or nsrc * ntap > 64:
        return False
    n0, n1 = r.shape
    with torch.cuda.device(r.device):
        plan = AcousticPlan(n0, n1, f.shape[0], ns, nsrc * ntap, nrec * ntap, 1, float(c0), float(c1),
                            r.device.index, 0, int(edge_rows))
        ok = plan.cluster_slabs() > 0
        plan.close()
    return ok


def _linearised(name, r, dr, f, q0, q1, src_cell, src_w, rec_cell, rec_w, c0, c1, cpml_width, snapshot_budget, adjoint,
                weight):
    """born / gauss_newton_product through :func:`_driver.linearised`.  Returns (rec, drec, hv); rec is None with
    ``adjoint``, hv without."""
    _require_cuda(r, "r")
    if tuple(dr.shape) != tuple(r.shape):
        raise MifwiError("dr must have the shape of r")
    rec, drec, hv = linearised(_Acoustic, name, r, dr, f, None, q0, q1, (src_cell, src_w, rec_cell, rec_w), snapshot_budget,
                               adjoint, weight, _options(c0, c1, 0, 0, cpml_width))
    return rec and rec[0], drec[0], hv


def born(r, f, dr, q0, q1, src_cell, src_w, rec_cell, rec_w, c0=1.0, c1=1.0,
         snapshot_budget=DEFAULT_SNAPSHOT_BUDGET, cpml_width=0):
    """Born / linearised modelling (``AcousticWaveSolver.born``, wavesolver.py:174-209;
    ``BornOperator``, operators.py:168-207): returns ``(rec, drec)`` where ``rec`` are the seismograms
    of the background model ``r`` and ``drec = J dr`` their first-order change for the perturbation
    ``dr`` (same parametrisation and shape as ``r``).  ``J`` is the exact transpose partner of the
    gradient autograd returns for :func:`propagate`.  No autograd through this call.

    The forward snapshots of all steps stay resident, within ``snapshot_budget`` and 80 % of the memory that is free.
    When the snapshots of all shots do not fit, the shots are taken a few at a time (they are independent: the same
    bits); when not even one shot fits, ``MifwiError`` - Born across time checkpoints is not served."""
    rec, drec, _ = _linearised("born", r, dr, f, q0, q1, src_cell, src_w, rec_cell, rec_w, c0, c1, cpml_width,
                               snapshot_budget, False, None)
    return rec, drec


def gauss_newton_product(r, dr, f, q0, q1, src_cell, src_w, rec_cell, rec_w, c0=1.0, c1=1.0, cpml_width=0, weight=None,
                         snapshot_budget=DEFAULT_SNAPSHOT_BUDGET):
    """Gauss-Newton Hessian-vector product ``hv = J^T W J dr`` [n0, n1] with ONE background forward, one Born pass
    (``mifwi_acoustic_born``) and one adjoint pass (``mifwi_acoustic_backward``) over the same resident snapshot buffer
    (composing :func:`born` and :func:`propagate` runs the background twice).  Returns ``(hv, drec)`` with
    ``drec = J dr`` [nt, nshot, nrec] as :func:`born` gives it.  Arguments as :func:`born`; no autograd through this call.

    ``weight``: None - the L2 misfit's identity - or a callable ``drec -> g``: a data weighting, or the second
    derivative of another misfit.  When the snapshots of all shots do not fit ``snapshot_budget`` the shots are taken a
    few at a time (they are independent); ``hv`` sums over the chunks and ``weight`` is then called once per chunk with
    that chunk's [nt, shots, nrec] traces, so it must act shot by shot.  When not even one shot fits, ``MifwiError``:
    Gauss-Newton products across time checkpoints are not served."""
    _, drec, hv = _linearised("gauss_newton_product", r, dr, f, q0, q1, src_cell, src_w, rec_cell, rec_w, c0, c1, cpml_width,
                              snapshot_budget, True, weight)
    return hv, drec
