"""Host side of the variable-density acoustic (fluid) propagator: the three material planes, plan and buffer handling
and the ``torch.autograd.Function`` around the HIP forward / adjoint of csrc/mifwi_fluid.hip.

Serves the DENISE runs with ``PHYSICS = 2`` of the reference's field-data path (models/networks.py:10445-10453) with
the fields an acoustic medium has - vx, vz and p - where :mod:`elastic` with Vs = 0 marches five.  Same grid, C-PML
tables, sources and receivers as :func:`elastic.propagate`, and the same seismograms bit for bit.  All wave arithmetic
is in libmifwi.so; there is no CPU path.
"""
import torch

from . import _lib, elastic
from ._lib import MifwiError
from ._driver import _Geometry, _Plan, _require_cuda, _stream, ptrs, run_backward, run_forward, segment_length
from .elastic import DEFAULT_SNAPSHOT_BUDGET, SOURCE_TYPES


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


def _forward_call(plan, coef, f_d, geo, rvx, rvz, rp):
    """``forward(snap_ptr, work_ptr, b, e, flags)`` as the drivers take it; no outputs: a re-run that samples nothing."""
    lib = _lib.load()
    args = (plan.handle, *coef, _lib.ptr(f_d), *geo, _lib.ptr(rvx), _lib.ptr(rvz), _lib.ptr(rp))
    return lambda snap, work, b, e, flags: _lib.check(lib.mifwi_fluid_forward(*args, snap, work, b, e, flags, _stream()))


class _FluidFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, mat, f, pz, px, geom, pml_width, shots_per_group, snapshot_budget, free_surface, source_type,
                record_pressure, fd_order):
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

            def adjoint(snap, first, hi, lo, flags):
                _lib.check(lib.mifwi_fluid_backward(plan.handle, *coef, *geo, *ptrs(*g), snap, first, _lib.ptr(grad_mat),
                                                    _lib.ptr(grad_f), _lib.ptr(work), hi, lo, flags, _stream()))
            run_backward("elastic", nt, ctx.seg, ctx.snap, adjoint, None,
                         _forward_call(plan, coef, f_d, geo, None, None, None), ctx.ckpt, lay, (lay.snap_step_elems,))
            plan.close()
            ctx.plan = ctx.snap = ctx.ckpt = None
        return (grad_mat[:, :, :nx].contiguous(), grad_f) + (None,) * 10


def propagate(mat, f, pz, px, src_cell, src_w, rec_cell, rec_w, pml_width, free_surface=False, source_type="explosive",
              record_pressure=False, fd_order=4, shots_per_group=0, snapshot_budget=DEFAULT_SNAPSHOT_BUDGET):
    """Acoustic forward modelling in a variable-density medium, differentiable w.r.t. ``mat`` and ``f``.

    mat [3,nz,nx] from :func:`materials`;  f [nt,nshot,nsrc]: added to p (``source_type`` "explosive"), or to vx / vz
    between the velocity and the pressure update ("fx" / "fz", DENISE QUELLTYP 2 / 3; scale it with
    :func:`force_amplitude`).  pz, px, cells, taps, ``pml_width``, ``free_surface`` (build ``mat`` with it), ``fd_order``,
    ``shots_per_group`` and ``snapshot_budget`` (time checkpointing when the snapshots do not fit) as in
    :func:`elastic.propagate`.  Returns (rec_vx, rec_vz), each [nt,nshot,nrec], and with ``record_pressure`` also
    rec_p = sum w (p + p): the elastic route's sxx + szz, DENISE's pressure seismogram is ``-rec_p``.
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
    rvx, rvz, rp = _FluidFn.apply(mat, f, pz, px, geom, int(pml_width), int(shots_per_group), int(snapshot_budget),
                                  1 if free_surface else 0, st, bool(record_pressure), int(fd_order))
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
