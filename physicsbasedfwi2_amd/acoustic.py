"""Host side of the acoustic propagator: plan handling, buffer allocation (torch = device
memory + stream plumbing only) and the ``torch.autograd.Function`` through which the model
gradient reaches the caller, as deepwave's autograd backward does at
models/networks.py:5464/5491 and ``FWILoss`` does at seisgan/fwi/layers.py:158-197.

All arithmetic happens in libmifwi.so (HIP); there is no CPU path here.
"""
import torch

from . import _lib
from ._lib import MifwiError
from ._driver import (_GEOMETRIES, _Geometry, _MomentsHolder, _Plan, _require_cuda, _stream,  # noqa: F401 (re-exported)
                      pad_columns, ptrs, run_backward, run_forward, segment_length)

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
        if self.moments is None:
            raise MifwiError("PseudoHessian.%s: no moments yet - run a backward pass through "
                             "propagate(..., pseudo_hessian=holder) first" % what)
        mom = self.moments.contiguous()
        n0, n1 = mom.shape
        pad = int(pad)
        nz, nx = n0 - 2 * pad, n1 - 2 * pad
        mdl = torch.as_tensor(model).detach().to(device=mom.device, dtype=torch.float32).contiguous()
        if pad < 0 or tuple(mdl.shape) != (nz, nx):
            raise MifwiError("PseudoHessian.%s: the model must be [%d, %d] (moments [%d, %d], pad %d), got %s"
                             % (what, nz, nx, n0, n1, pad, tuple(mdl.shape)))
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
    """``forward(snap_ptr, work_ptr, b, e, flags)`` as the drivers take it; ``rec`` None: a re-run that samples nothing."""
    lib = _lib.load()
    args = (plan.handle, *coef, _lib.ptr(f_d), *geo, _lib.ptr(rec))
    return lambda snap, work, b, e, flags: _lib.check(
        lib.mifwi_acoustic_forward(*args, snap, work, b, e, flags, _stream()))


def _adjoint_call(plan, coef, geo, g, grad_r, grad_f, work):
    """``adjoint(snap_ptr, snap_first, hi, lo, flags)`` as the backward driver takes it."""
    lib = _lib.load()
    return lambda snap, first, hi, lo, flags: _lib.check(lib.mifwi_acoustic_backward(
        plan.handle, *coef, *geo, _lib.ptr(g), snap, first, _lib.ptr(grad_r), _lib.ptr(grad_f), _lib.ptr(work), hi, lo,
        flags, _stream()))


class _AcousticFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, r, f, q0, q1, geom, c0, c1, shots_per_group, snapshot_budget, edge_rows, cpml_width=0,
                pseudo_hessian=None):
        _require_cuda(r, "r")
        dev = r.device
        n0, n1 = r.shape
        nt, ns, nsrc = f.shape
        if geom.src_cell.shape[:2] != (ns, nsrc):
            raise MifwiError("f is [nt,%d,%d] but src_cell is %s" % (ns, nsrc,
                                                                      tuple(geom.src_cell.shape)))
        nrec, ntap = geom.rec_cell.shape[1], geom.rec_cell.shape[2]
        geom.check_cells(n0 * n1, "%dx%d" % (n0, n1))
        with torch.cuda.device(dev):
            plan = AcousticPlan(n0, n1, nt, ns, nsrc, nrec, ntap, c0, c1, dev.index,
                                shots_per_group, edge_rows, cpml_width)
            lay = plan.layout
            r_p, q0_d, q1_p = _acoustic_inputs(r, q0, q1, cpml_width, lay.gp)
            f_d = f.detach().to(dtype=torch.float32).contiguous()
            rec = torch.empty((nt, ns, nrec), device=dev, dtype=torch.float32)
            work = torch.empty(lay.work_forward_elems, device=dev, dtype=torch.float32)
            need_grad = r.requires_grad or f.requires_grad
            if pseudo_hessian is not None and not need_grad:
                raise MifwiError("pseudo_hessian: the moments are taken from the snapshots of a backward pass, and "
                                 "neither r nor f requires a gradient in this run")
            seg, snap = nt, None
            if need_grad:
                seg = segment_length(snapshot_budget, dev, 4 * ns * lay.coef_elems, nt)
                if seg == nt:
                    snap = torch.empty((nt, ns, n0, lay.gp), device=dev, dtype=torch.float32)
            geo = ptrs(geom.src_cell, geom.src_w, geom.rec_cell, geom.rec_w)
            ckpt = run_forward(_forward_call(plan, ptrs(r_p, q0_d, q1_p), f_d, geo, rec), nt, seg, work,
                               lay.state_elems, snap)
            if need_grad:
                ctx.plan = plan
                ctx.geom = geom
                ctx.seg = seg
                ctx.ckpt = ckpt
                ctx.snap = snap
                ctx.dims = (n0, n1, nt, ns, nsrc, nrec)
                ctx.need_f = f.requires_grad
                ctx.hess = pseudo_hessian
                ctx.save_for_backward(r_p, q0_d, q1_p, f_d)
            else:
                plan.close()
        return rec

    @staticmethod
    def backward(ctx, grad_rec):
        lib = _lib.load()
        if ctx.plan is None:
            raise MifwiError("backward through the acoustic propagator was called twice: the forward snapshots "
                             "(or checkpoints) are freed by the first call - run the forward again")
        r_p, q0_d, q1_p, f_d = ctx.saved_tensors
        plan, geom = ctx.plan, ctx.geom
        lay = plan.layout
        n0, n1, nt, ns, nsrc, nrec = ctx.dims
        dev = r_p.device
        with torch.cuda.device(dev):
            g = grad_rec.to(dtype=torch.float32).contiguous()
            grad_r = torch.empty((n0, lay.gp), device=dev, dtype=torch.float32)
            grad_f = (torch.zeros((nt, ns, nsrc), device=dev, dtype=torch.float32)
                      if ctx.need_f else None)
            work = torch.empty(lay.work_backward_elems, device=dev, dtype=torch.float32)
            hess = ctx.hess
            moments = None
            if hess is not None:
                mom = torch.zeros((n0, lay.gp), device=dev, dtype=torch.float32)
                mwork = torch.empty(lib.mifwi_acoustic_snapshot_moments_work_elems(plan.handle), device=dev,
                                    dtype=torch.float32)

                def moments(snap, first, b, e):
                    # one more read of a snapshot range this pass has in hand, each range once (absolute step numbers, so
                    # segments select the steps the resident buffer would); G^{nt-1} never reaches a recorded sample
                    _lib.check(lib.mifwi_acoustic_snapshot_moments(
                        plan.handle, snap, first, b, e, hess.stride, _lib.ptr(mom), _lib.ptr(mwork), 0, _stream()))
            coef = ptrs(r_p, q0_d, q1_p)
            geo = ptrs(geom.src_cell, geom.src_w, geom.rec_cell, geom.rec_w)
            if nt < 2:                           # no adjoint step, so no visit: nothing writes the gradient
                grad_r.zero_()
            run_backward("acoustic", nt, ctx.seg, ctx.snap, _adjoint_call(plan, coef, geo, g, grad_r, grad_f, work), moments,
                         _forward_call(plan, coef, f_d, geo, None), ctx.ckpt, lay, (ns, n0, lay.gp))
            if hess is not None:
                hess._add(mom[:, :n1])
                ctx.hess = None
            plan.close()
            ctx.plan = None
            ctx.snap = None
            ctx.ckpt = None
        return (grad_r[:, :n1].contiguous(), grad_f) + (None,) * 10


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
        rec = _AcousticFn.apply(r, f.repeat_interleave(ntap, dim=2), q0, q1, flat, float(c0), float(c1),
                                int(shots_per_group), int(snapshot_budget), int(edge_rows), 0, pseudo_hessian)
        return rec.reshape(rec.shape[0], ns, nrec, ntap).sum(dim=3)
    return _AcousticFn.apply(r, f, q0, q1, geom, float(c0), float(c1), int(shots_per_group),
                             int(snapshot_budget), int(edge_rows), int(cpml_width), pseudo_hessian)


def _flatten_taps_pays(r, f, geom, c0, c1, edge_rows):
    """True when the flattened (single-tap) problem runs on the single-launch kernels' fast paths."""
    import os
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
    """born / gauss_newton_product: per shot chunk one plan, one background forward with resident snapshots, the Born
    pass over that buffer and - ``adjoint`` - the adjoint pass over it too.  Returns (rec, drec, hv); rec is None with
    ``adjoint``, hv without."""
    _require_cuda(r, "r")
    dev = r.device
    lib = _lib.load()
    geom = _Geometry.get(src_cell, src_w, rec_cell, rec_w, dev)
    n0, n1 = r.shape
    nt, ns, nsrc = f.shape
    if geom.src_cell.shape[:2] != (ns, nsrc):
        raise MifwiError("f is [nt,%d,%d] but src_cell is %s" % (ns, nsrc, tuple(geom.src_cell.shape)))
    nrec, ntap = geom.rec_cell.shape[1], geom.rec_cell.shape[2]
    if tuple(dr.shape) != (n0, n1):
        raise MifwiError("dr must have the shape of r")
    geom.check_cells(n0 * n1, "%dx%d" % (n0, n1))
    with torch.cuda.device(dev), torch.no_grad():
        gp = 4 * ((n1 + 3) // 4)
        budget = min(int(snapshot_budget), int(0.8 * _lib.free_device_bytes(dev)))
        chunk = min(ns, budget // (4 * nt * n0 * gp))
        if chunk < 1:
            raise MifwiError("%s keeps the forward snapshots of all %d steps resident, and not even one shot's fit the "
                             "snapshot budget; products across time checkpoints are not served" % (name, nt))
        r_p, q0_d, q1_p = _acoustic_inputs(r, q0, q1, cpml_width, gp)
        dr_p = pad_columns(dr.to(dev), gp)
        f_d = f.detach().to(device=dev, dtype=torch.float32).contiguous()
        rec = None if adjoint else torch.empty((nt, ns, nrec), device=dev, dtype=torch.float32)
        drec = torch.empty((nt, ns, nrec), device=dev, dtype=torch.float32)
        hv = torch.zeros((n0, n1), device=dev, dtype=torch.float32) if adjoint else None
        coef = ptrs(r_p, q0_d, q1_p)
        # Born modelling of all shots at once writes its outputs in place; a product's traces stay the chunk's own tensor,
        # which is what the caller's weight() gets
        in_place = chunk == ns and not adjoint
        for a in range(0, ns, chunk):
            c = min(chunk, ns - a)
            sl = slice(a, a + c)
            plan = AcousticPlan(n0, n1, nt, c, nsrc, nrec, ntap, float(c0), float(c1), dev.index, 0, 0, int(cpml_width))
            try:
                lay = plan.layout
                taps = [t[sl].contiguous() for t in (geom.src_cell, geom.src_w, geom.rec_cell, geom.rec_w)]
                geo = ptrs(*taps)
                fc = f_d[:, sl].contiguous()
                rec_c, drc = (rec, drec) if in_place else (
                    torch.empty((nt, c, nrec), device=dev, dtype=torch.float32) for _ in range(2))
                work = torch.empty(max(lay.work_forward_elems, lay.work_backward_elems if adjoint else 0), device=dev,
                                   dtype=torch.float32)
                snap = torch.empty((nt, c, n0, gp), device=dev, dtype=torch.float32)
                run_forward(_forward_call(plan, coef, fc, geo, rec_c), nt, nt, work, lay.state_elems, snap)
                _lib.check(lib.mifwi_acoustic_born(plan.handle, *coef, _lib.ptr(dr_p), geo[2], geo[3], _lib.ptr(snap), 0,
                                                   _lib.ptr(drc), _lib.ptr(work), 0, nt, _lib.ZERO_STATE, _stream()))
                if not in_place:
                    drec[:, sl] = drc
                    if rec is not None:
                        rec[:, sl] = rec_c
                if adjoint and nt >= 2:
                    g = drc if weight is None else weight(drc)
                    g = g.detach().to(device=dev, dtype=torch.float32).contiguous()
                    if g.shape != drc.shape:
                        raise MifwiError("weight must return a tensor of the shape of its argument")
                    grad = torch.empty((n0, gp), device=dev, dtype=torch.float32)
                    run_backward("acoustic", nt, nt, snap, _adjoint_call(plan, coef, geo, g, grad, None, work))
                    hv += grad[:, :n1]
            finally:
                plan.close()
    return rec, drec, hv


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
