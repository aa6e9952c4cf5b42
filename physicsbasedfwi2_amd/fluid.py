"""Host side of the variable-density acoustic (fluid) propagator: the three material planes, plan and buffer handling
and the ``torch.autograd.Function`` around the HIP forward / adjoint of csrc/mifwi_fluid.hip.

Serves the DENISE runs with ``PHYSICS = 2`` of the reference's field-data path (models/networks.py:10445-10453) with
the fields an acoustic medium has - vx, vz and p - where :mod:`elastic` with Vs = 0 marches five.  Same grid, C-PML
tables, sources and receivers as :func:`elastic.propagate`, and the same seismograms bit for bit.  Beyond the gradient:
Born modelling and Gauss-Newton products (:func:`born`, :func:`gauss_newton_product`, :func:`materials_jvp`) and the
diagonal pseudo-Hessian (:class:`PseudoHessian`), the counterparts of the elastic ones.  All wave arithmetic is in
libmifwi.so; there is no CPU path.
"""
import torch

from . import _lib, elastic
from ._lib import MifwiError
from ._driver import (_Geometry, _MomentsHolder, _Plan, _require_cuda, _stream, pad_columns, ptrs, run_backward,
                      run_forward, segment_length)
from .elastic import DEFAULT_SNAPSHOT_BUDGET, PARAM_IMPEDANCE, PARAM_LAME, PARAM_VELOCITY, SOURCE_TYPES  # noqa: F401


def materials(vp, rho, dt, h, free_surface=False):
    """[3, nz, nx] = K dt/h, dt/(h rho_x), dt/(h rho_z) with K = rho Vp^2: planes 0, 3 and 4 of
    ``elastic.staggered_materials(vp, 0, rho)`` - the same bits, differentiable through the same kernels.  Under
    ``free_surface`` row 0 of K is 0 (p = 0 there)."""
    m5 = elastic.staggered_materials(vp, torch.zeros_like(vp), rho, dt, h)
    K = m5[0]
    if free_surface:
        keep = torch.ones_like(K)
        keep[0] = 0.0
        K = K * keep
    return torch.stack([K, m5[3], m5[4]])


class FluidPlan(_Plan):
    PREFIX, LAYOUT = "fluid", _lib.FluidLayout

    def __init__(self, nz, nx, nt, nshot, nsrc, nrec, ntap, pml_width, device_index, shots_per_group=0, free_surface=0,
                 source_type=0, fd_order=4):
        self._create(_lib.FluidDesc(nz, nx, nt, nshot, nsrc, nrec, ntap, pml_width, free_surface, shots_per_group,
                                    source_type, fd_order), device_index)


class PseudoHessian(_MomentsHolder):
    """Holder of the three snapshot second moments behind the diagonal pseudo-Hessian of the fluid gradient (DENISE's
    ``EPRECOND = 1``), the counterpart of :class:`elastic.PseudoHessian`: pass it to :func:`propagate`
    (``pseudo_hessian=``) and every backward pass through that call adds ``M0 = sum S0^2, M1 = sum S1^2, M2 = sum S2^2``
    of its forward snapshot planes - summed over its shots and over the steps n with ``n % stride == 0``, each weighted
    by ``stride`` - into ``.moments`` [3, nz, nx] (None before the first backward).  The holder accumulates over calls
    (shot chunks, ranks' shares); :meth:`reset` zeroes it.  One more read of the snapshot buffer the backward holds
    (``mifwi_fluid_snapshot_moments``), no extra propagation."""

    def hessian(self, vp, rho, dt, h, parametrization=PARAM_VELOCITY):
        """[2, nz, nx]: the pseudo-Hessian planes of (Vp, rho), (Zp, rho) or (K, rho) from the moments held and the
        model the run used: ``H_p = 2 K_p^2 M0 + b_p^2 (M1 + M2)`` (include/mifwi.h has the table) - planes 0 and 2 of
        ``elastic.PseudoHessian.hessian(vp, 0, rho, ...)`` of the elastic route's run.  Finite and >= 0 everywhere."""
        if self.moments is None:
            raise MifwiError("PseudoHessian.hessian: no moments yet - run a backward pass through "
                             "propagate(..., pseudo_hessian=holder) first")
        mom = self.moments.contiguous()
        _, nz, nx = mom.shape
        prm = [torch.as_tensor(t).detach().to(device=mom.device, dtype=torch.float32).contiguous() for t in (vp, rho)]
        if any(tuple(t.shape) != (nz, nx) for t in prm):
            raise MifwiError("PseudoHessian.hessian: the model must be [%d, %d] like the moments" % (nz, nx))
        out = torch.empty((2, nz, nx), device=mom.device, dtype=torch.float32)
        with torch.cuda.device(mom.device):
            _lib.check(_lib.load().mifwi_fluid_pseudo_hessian(
                mom.device.index or 0, int(parametrization), _lib.ptr(prm[0]), _lib.ptr(prm[1]), _lib.ptr(mom), nz, nx, nx,
                float(dt) / float(h), _lib.ptr(out[0]), _lib.ptr(out[1]), _stream()))
        return out


def _forward_call(plan, coef, f_d, geo, rvx, rvz, rp):
    """``forward(snap_ptr, work_ptr, b, e, flags)`` as the drivers take it; no outputs: a re-run that samples nothing."""
    lib = _lib.load()
    args = (plan.handle, *coef, _lib.ptr(f_d), *geo, _lib.ptr(rvx), _lib.ptr(rvz), _lib.ptr(rp))
    return lambda snap, work, b, e, flags: _lib.check(lib.mifwi_fluid_forward(*args, snap, work, b, e, flags, _stream()))


def _adjoint_call(plan, coef, geo, g, grad_mat, grad_f, work):
    """``adjoint(snap_ptr, snap_first, hi, lo, flags)`` as the backward driver takes it; g = (g_vx, g_vz, g_p), each a
    tensor or None."""
    lib = _lib.load()
    return lambda snap, first, hi, lo, flags: _lib.check(lib.mifwi_fluid_backward(
        plan.handle, *coef, *geo, *ptrs(*g), snap, first, _lib.ptr(grad_mat), _lib.ptr(grad_f), _lib.ptr(work), hi, lo,
        flags, _stream()))


class _FluidFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mat, f, pz, px, geom, pml_width, shots_per_group, snapshot_budget, free_surface, source_type,
                record_pressure, fd_order, pseudo_hessian=None):
        dev = mat.device
        _, nz, nx = mat.shape
        nt, ns, nsrc = f.shape
        if geom.src_cell.shape[:2] != (ns, nsrc):
            raise MifwiError("f is [nt,%d,%d] but src_cell is %s" % (ns, nsrc, tuple(geom.src_cell.shape)))
        nrec, ntap = geom.rec_cell.shape[1], geom.rec_cell.shape[2]
        geom.check_cells(nz * nx, "%dx%d" % (nz, nx))
        with torch.cuda.device(dev):
            plan = FluidPlan(nz, nx, nt, ns, nsrc, nrec, ntap, pml_width, dev.index, shots_per_group, free_surface,
                             source_type, fd_order)
            lay = plan.layout
            mat_p, pz_d, px_p = elastic._padded_inputs(mat, pz, px, lay.gp)
            f_d = f.detach().to(dtype=torch.float32).contiguous()
            rvx = torch.empty((nt, ns, nrec), device=dev, dtype=torch.float32)
            rvz = torch.empty((nt, ns, nrec), device=dev, dtype=torch.float32)
            rp = torch.empty((nt, ns, nrec), device=dev, dtype=torch.float32) if record_pressure else None
            work = torch.empty(lay.work_forward_elems, device=dev, dtype=torch.float32)
            need_grad = mat.requires_grad or f.requires_grad
            if pseudo_hessian is not None and not need_grad:
                raise MifwiError("pseudo_hessian: the moments are taken from the snapshots of a backward pass, and "
                                 "neither mat nor f requires a gradient in this run")
            seg, snap = nt, None
            if need_grad:
                seg = segment_length(snapshot_budget, dev, 4 * lay.snap_step_elems, nt)
                if seg == nt:
                    snap = torch.empty((nt, lay.snap_step_elems), device=dev, dtype=torch.float32)
            geo = ptrs(geom.src_cell, geom.src_w, geom.rec_cell, geom.rec_w)
            ckpt = run_forward(_forward_call(plan, ptrs(mat_p, pz_d, px_p), f_d, geo, rvx, rvz, rp), nt, seg, work,
                               lay.state_elems, snap)
            if need_grad:
                ctx.plan, ctx.geom, ctx.seg, ctx.ckpt, ctx.snap = plan, geom, seg, ckpt, snap
                ctx.dims = (nz, nx, nt, ns, nsrc, nrec)
                ctx.need_f = f.requires_grad
                ctx.hess = pseudo_hessian
                ctx.save_for_backward(mat_p, pz_d, px_p, f_d)
            else:
                plan.close()
        return rvx, rvz, (rp if record_pressure else torch.empty(0, device=dev))

    @staticmethod
    def backward(ctx, g_vx, g_vz, g_p=None):
        lib = _lib.load()
        if ctx.plan is None:
            raise MifwiError("backward through the fluid propagator was called twice: the forward snapshots "
                             "(or checkpoints) are freed by the first call - run the forward again")
        mat_p, pz_d, px_p, f_d = ctx.saved_tensors
        plan, geom = ctx.plan, ctx.geom
        lay = plan.layout
        nz, nx, nt, ns, nsrc, nrec = ctx.dims
        dev = mat_p.device
        with torch.cuda.device(dev):
            g = [None if t is None or t.numel() == 0 else t.to(dtype=torch.float32).contiguous() for t in (g_vx, g_vz, g_p)]
            grad_mat = torch.empty((3, nz, lay.gp), device=dev, dtype=torch.float32)
            grad_f = torch.zeros((nt, ns, nsrc), device=dev, dtype=torch.float32) if ctx.need_f else None
            work = torch.empty(lay.work_backward_elems, device=dev, dtype=torch.float32)
            coef = ptrs(mat_p, pz_d, px_p)
            geo = ptrs(geom.src_cell, geom.src_w, geom.rec_cell, geom.rec_w)
            hess = ctx.hess
            moments = None
            if hess is not None:
                mom = torch.empty((3, nz, lay.gp), device=dev, dtype=torch.float32)
                mwork = torch.empty(lib.mifwi_fluid_snapshot_moments_work_elems(plan.handle), device=dev,
                                    dtype=torch.float32)

                def moments(snap, first, b, e):
                    # one more read of a snapshot range this pass has in hand, each range once (absolute step numbers, so
                    # segments select the steps the resident buffer would); the range that ends the run comes first
                    _lib.check(lib.mifwi_fluid_snapshot_moments(
                        plan.handle, snap, first, b, e, hess.stride, _lib.ptr(mom), _lib.ptr(mwork),
                        _lib.ZERO_STATE if e == nt else 0, _stream()))
            run_backward("elastic", nt, ctx.seg, ctx.snap, _adjoint_call(plan, coef, geo, g, grad_mat, grad_f, work), moments,
                         _forward_call(plan, coef, f_d, geo, None, None, None), ctx.ckpt, lay, (lay.snap_step_elems,))
            if hess is not None:
                hess._add(mom[:, :, :nx])
                ctx.hess = None
            plan.close()
            ctx.plan = ctx.snap = ctx.ckpt = None
        return (grad_mat[:, :, :nx].contiguous(), grad_f) + (None,) * 11


def propagate(mat, f, pz, px, src_cell, src_w, rec_cell, rec_w, pml_width, free_surface=False, source_type="explosive",
              record_pressure=False, fd_order=4, shots_per_group=0, snapshot_budget=DEFAULT_SNAPSHOT_BUDGET,
              pseudo_hessian=None):
    """Acoustic forward modelling in a variable-density medium, differentiable w.r.t. ``mat`` and ``f``.

    mat [3,nz,nx] from :func:`materials`;  f [nt,nshot,nsrc]: added to p (``source_type`` "explosive"), or to vx / vz
    between the velocity and the pressure update ("fx" / "fz", DENISE QUELLTYP 2 / 3; scale it with
    :func:`force_amplitude`).  pz, px, cells, taps, ``pml_width``, ``free_surface`` (build ``mat`` with it), ``fd_order``,
    ``shots_per_group`` and ``snapshot_budget`` (time checkpointing when the snapshots do not fit) as in
    :func:`elastic.propagate`.  Returns (rec_vx, rec_vz), each [nt,nshot,nrec], and with ``record_pressure`` also
    rec_p = sum w (p + p): the elastic route's sxx + szz, DENISE's pressure seismogram is ``-rec_p``.
    pseudo_hessian: a :class:`PseudoHessian` holder, or None.  The backward pass through this call then adds the second
    moments of its snapshot planes into the holder (one more read of the snapshot buffer - resident, or every
    regenerated checkpoint segment once); a run that needs no gradient has no such pass and raises.  Without a holder
    nothing changes: the same launches, the same results.
    The seismograms equal those of :func:`elastic.propagate` on ``staggered_materials(vp, 0, rho)`` bit for bit (within
    rounding of the surface row under ``free_surface``).  One launch per half step; repeated calls return the same bits
    while no cell receives more than two receiver taps of a shot - more than one, when the backward pass gets pressure
    adjoint sources (they are added to the adjoint p with global float atomics)."""
    _require_cuda(mat, "mat")
    if mat.dim() != 3 or mat.shape[0] != 3:
        raise MifwiError("mat must be [3, nz, nx] (fluid.materials)")
    geom = _Geometry.get(src_cell, src_w, rec_cell, rec_w, mat.device)
    f = f.to(device=mat.device)
    try:
        st = SOURCE_TYPES[source_type]
    except KeyError:
        raise MifwiError("source_type must be one of %s" % sorted(k for k in SOURCE_TYPES if isinstance(k, str)))
    if pseudo_hessian is not None and not isinstance(pseudo_hessian, PseudoHessian):
        raise MifwiError("pseudo_hessian must be a fluid.PseudoHessian holder or None")
    rvx, rvz, rp = _FluidFn.apply(mat, f, pz, px, geom, int(pml_width), int(shots_per_group), int(snapshot_budget),
                                  1 if free_surface else 0, st, bool(record_pressure), int(fd_order), pseudo_hessian)
    return (rvx, rvz, rp) if record_pressure else (rvx, rvz)


def force_amplitude(wavelet, mat, src_cell, src_w, h, source_type):
    """Point-force amplitudes for :func:`propagate`: wavelet [nt,nshot,nsrc] times dt/(h^2 rho) at the source node, with
    mat[1] = dt/(h rho_x), mat[2] = dt/(h rho_z) - :func:`elastic.force_amplitude` on the fluid's planes (the same bits).
    Differentiable w.r.t. ``mat``."""
    plane = mat[1 if SOURCE_TYPES[source_type] == 1 else 2].reshape(-1)
    cell = src_cell.to(device=mat.device, dtype=torch.long).clamp_min(0)
    w = src_w.to(device=mat.device, dtype=mat.dtype) * (src_cell.to(mat.device) >= 0)
    b = (plane[cell] * w).sum(dim=-1)                       # [nshot, nsrc]
    return wavelet.to(device=mat.device, dtype=mat.dtype) * (b / h)[None]


def materials_jvp(vp, rho, dvp, drho, dt, h, free_surface=False):
    """dmat [3, nz, nx]: the first-order change of :func:`materials` for the model perturbation (dvp, drho) - planes 0, 3
    and 4 of ``elastic.materials_jvp(vp, 0, rho, dvp, 0, drho, ...)``, the transpose of the VJP autograd runs through
    :func:`materials`.  Under ``free_surface`` row 0 of plane 0 is 0, as row 0 of K is."""
    vp = torch.as_tensor(vp).detach()
    zero = torch.zeros_like(vp)
    d5 = elastic.materials_jvp(vp, zero, rho, dvp, zero, drho, dt, h)
    dK = d5[0]
    if free_surface:
        dK = dK.clone()
        dK[0] = 0.0
    return torch.stack([dK, d5[3], d5[4]])


def _linearised(name, mat, dmat, f, pz, px, src_cell, src_w, rec_cell, rec_w, pml_width, df, free_surface, source_type,
                record_pressure, fd_order, snapshot_budget, adjoint, weight):
    """born / gauss_newton_product, on the pattern of ``elastic._linearised``: per shot chunk one plan, one background
    forward with resident snapshots, the Born pass over that buffer and - ``adjoint`` - the adjoint pass over it too.
    Returns (background traces, perturbed traces, hv): two lists of 2 or 3 tensors."""
    _require_cuda(mat, "mat")
    dev = mat.device
    lib = _lib.load()
    geom = _Geometry.get(src_cell, src_w, rec_cell, rec_w, dev)
    try:
        st = SOURCE_TYPES[source_type]
    except KeyError:
        raise MifwiError("source_type must be one of %s" % sorted(k for k in SOURCE_TYPES if isinstance(k, str)))
    if mat.dim() != 3 or mat.shape[0] != 3:
        raise MifwiError("mat must be [3, nz, nx] (fluid.materials)")
    if tuple(dmat.shape) != tuple(mat.shape):
        raise MifwiError("dmat must have the shape of mat, %s (got %s)" % (tuple(mat.shape), tuple(dmat.shape)))
    _require_cuda(dmat, "dmat")
    _, nz, nx = mat.shape
    nt, ns, nsrc = f.shape
    if geom.src_cell.shape[:2] != (ns, nsrc):
        raise MifwiError("f is [nt,%d,%d] but src_cell is %s" % (ns, nsrc, tuple(geom.src_cell.shape)))
    if df is not None and tuple(df.shape) != tuple(f.shape):
        raise MifwiError("df must have the shape of f, %s (got %s)" % (tuple(f.shape), tuple(df.shape)))
    nrec, ntap = geom.rec_cell.shape[1], geom.rec_cell.shape[2]
    geom.check_cells(nz * nx, "%dx%d" % (nz, nx))
    ntr = 3 if record_pressure else 2
    fs = 1 if free_surface else 0

    def make_plan(c):
        return FluidPlan(nz, nx, nt, c, nsrc, nrec, ntap, int(pml_width), dev.index, 0, fs, st, int(fd_order))
    with torch.cuda.device(dev), torch.no_grad():
        f_d = f.detach().to(device=dev, dtype=torch.float32).contiguous()
        df_d = None if df is None else df.detach().to(device=dev, dtype=torch.float32).contiguous()
        rec = [torch.empty((nt, ns, nrec), device=dev, dtype=torch.float32) for _ in range(ntr)]
        drec = [torch.empty((nt, ns, nrec), device=dev, dtype=torch.float32) for _ in range(ntr)]
        hv = torch.zeros((3, nz, nx), device=dev, dtype=torch.float32) if adjoint else None
        budget = min(int(snapshot_budget), int(0.8 * _lib.free_device_bytes(dev)))
        one = make_plan(1)
        chunk = min(ns, budget // (4 * nt * one.layout.snap_step_elems))     # the planes of a step are per shot
        one.close()
        if chunk < 1:
            raise MifwiError("%s keeps the forward snapshots of all %d steps resident, and not even one shot's fit "
                             "the snapshot budget; Born modelling across time checkpoints is not served" % (name, nt))
        for a in range(0, ns, chunk):
            c = min(chunk, ns - a)
            plan = make_plan(c)
            try:
                lay = plan.layout
                sl = slice(a, a + c)
                mat_p, pz_d, px_p = elastic._padded_inputs(mat, pz, px, lay.gp)
                dmat_p = pad_columns(dmat.to(dev), lay.gp)
                taps = [t[sl].contiguous() for t in (geom.src_cell, geom.src_w, geom.rec_cell, geom.rec_w)]
                geo = ptrs(*taps)
                fc = f_d[:, sl].contiguous()
                dfc = None if df_d is None else df_d[:, sl].contiguous()
                r, dr = ([torch.empty((nt, c, nrec), device=dev, dtype=torch.float32) for _ in range(ntr)] + [None] * (3 - ntr)
                         for _ in range(2))
                work = torch.empty(max(lay.work_forward_elems, lay.work_backward_elems if adjoint else 0), device=dev,
                                   dtype=torch.float32)
                snap = torch.empty((nt, lay.snap_step_elems), device=dev, dtype=torch.float32)
                coef = ptrs(mat_p, pz_d, px_p)
                run_forward(_forward_call(plan, coef, fc, geo, *r), nt, nt, work, lay.state_elems, snap)
                _lib.check(lib.mifwi_fluid_born(plan.handle, coef[0], _lib.ptr(dmat_p), *coef[1:], _lib.ptr(dfc), *geo,
                                                _lib.ptr(snap), 0, *ptrs(*dr), _lib.ptr(work), 0, nt, _lib.ZERO_STATE,
                                                _stream()))
                for k in range(ntr):
                    rec[k][:, sl] = r[k]
                    drec[k][:, sl] = dr[k]
                if adjoint:
                    g = tuple(dr[:ntr]) if weight is None else weight(*dr[:ntr])
                    g = [t.detach().to(device=dev, dtype=torch.float32).contiguous() for t in g]
                    if len(g) != ntr or any(t.shape != dr[0].shape for t in g):
                        raise MifwiError("weight must return %d tensors of the shape of its arguments" % ntr)
                    grad = torch.empty((3, nz, lay.gp), device=dev, dtype=torch.float32)
                    run_backward("elastic", nt, nt, snap,
                                 _adjoint_call(plan, coef, geo, g + [None] * (3 - ntr), grad, None, work))
                    hv += grad[:, :, :nx]
            finally:
                plan.close()
    return rec, drec, hv


def born(mat, dmat, f, pz, px, src_cell, src_w, rec_cell, rec_w, pml_width, df=None, free_surface=False,
         source_type="explosive", record_pressure=False, fd_order=4, snapshot_budget=DEFAULT_SNAPSHOT_BUDGET):
    """Born / linearised modelling with the fluid kernels: returns ``(rec_vx, rec_vz[, rec_p], drec_vx, drec_vz[, drec_p])``
    - the seismograms of the background ``mat`` (what :func:`propagate` returns, bit for bit) and ``drec = J (dmat, df)``,
    their first-order change for the perturbation ``dmat`` [3, nz, nx] of the material planes (:func:`materials_jvp` maps
    (dVp, drho) to it) and, optionally, ``df`` [nt, nshot, nsrc] of the source amplitudes - injected where ``f`` is for
    every ``source_type``; the derivative of :func:`force_amplitude` is the caller's (a torch expression).  ``J`` is the
    exact transpose partner of the gradients autograd returns for :func:`propagate`.  No autograd through this call.

    One plan runs the background forward with resident snapshots; the Born pass (``mifwi_fluid_born``, the forward's two
    launches per step on the perturbed state) reads the same buffer.  When the snapshots of all shots do not fit
    ``snapshot_budget`` the shots are taken a few at a time (they are independent: the same bits); when not even one
    shot fits, ``MifwiError`` - Born across time checkpoints is not served."""
    rec, drec, _ = _linearised("born", mat, dmat, f, pz, px, src_cell, src_w, rec_cell, rec_w, pml_width, df, free_surface,
                               source_type, record_pressure, fd_order, snapshot_budget, False, None)
    return tuple(rec) + tuple(drec)


def gauss_newton_product(mat, dmat, f, pz, px, src_cell, src_w, rec_cell, rec_w, pml_width, df=None, free_surface=False,
                         source_type="explosive", record_pressure=False, fd_order=4,
                         snapshot_budget=DEFAULT_SNAPSHOT_BUDGET, weight=None):
    """Gauss-Newton Hessian-vector product ``hv = J^T W J dmat`` [3, nz, nx] with ONE background forward, one Born pass
    and one adjoint pass over the same resident snapshot buffer.  Returns ``(hv, drec_vx, drec_vz[, drec_p])`` with
    ``drec = J (dmat, df)`` as :func:`born` gives it.

    ``weight``: None - the L2 misfit's identity - or a callable ``(drec_vx, drec_vz[, drec_p]) -> (g_vx, g_vz[, g_p])``: a
    data weighting, or the second derivative of another misfit.  Shots are taken a few at a time like :func:`born` when
    their snapshots do not fit the budget; ``hv`` sums over the chunks and ``weight`` is then called once per chunk with
    that chunk's [nt, shots, nrec] traces, so it must act shot by shot.  Other arguments and refusals as :func:`born`."""
    _, drec, hv = _linearised("gauss_newton_product", mat, dmat, f, pz, px, src_cell, src_w, rec_cell, rec_w, pml_width,
                              df, free_surface, source_type, record_pressure, fd_order, snapshot_budget, True, weight)
    return (hv,) + tuple(drec)
