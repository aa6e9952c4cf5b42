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
from ._driver import _Geometry, _MomentsHolder, _Plan, _require_cuda, _stream, Physics, Propagate, linearised, ptrs
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
        mom = self._held("hessian")
        _, nz, nx = mom.shape
        prm = self._model_planes("hessian", mom, (vp, rho), (nz, nx))
        out = torch.empty((2, nz, nx), device=mom.device, dtype=torch.float32)
        with torch.cuda.device(mom.device):
            _lib.check(_lib.load().mifwi_fluid_pseudo_hessian(
                mom.device.index or 0, int(parametrization), _lib.ptr(prm[0]), _lib.ptr(prm[1]), _lib.ptr(mom), nz, nx, nx,
                float(dt) / float(h), _lib.ptr(out[0]), _lib.ptr(out[1]), _stream()))
        return out


def _three(tensors):
    """Device pointers of (vx, vz[, p]) traces, NULL for a missing one."""
    return ptrs(*(list(tensors or ()) + [None] * 3)[:3])


def _calls(prefix):
    """(forward_call, adjoint_call, born_call) around the entry points ``mifwi_<prefix>_forward`` / ``_backward`` / ``_born``:
    the lossless and the viscoacoustic family (:mod:`viscofluid`) take the same argument lists."""

    def forward_call(plan, coef, f_d, geo, rec):
        """``forward(snap_ptr, work_ptr, b, e, flags)`` as the drivers take it; rec = [rec_vx, rec_vz[, rec_p]], or None: a
        re-run that samples nothing."""
        fn = getattr(_lib.load(), "mifwi_%s_forward" % prefix)
        args = (plan.handle, *coef, _lib.ptr(f_d), *geo, *_three(rec))
        return lambda snap, work, b, e, flags: _lib.check(fn(*args, snap, work, b, e, flags, _stream()))

    def adjoint_call(plan, coef, geo, g, grad_mat, grad_f, work):
        """``adjoint(snap_ptr, snap_first, hi, lo, flags)`` as the backward driver takes it; g = [g_vx, g_vz[, g_p]], each a
        tensor or None."""
        fn = getattr(_lib.load(), "mifwi_%s_backward" % prefix)
        return lambda snap, first, hi, lo, flags: _lib.check(fn(
            plan.handle, *coef, *geo, *_three(g), snap, first, _lib.ptr(grad_mat), _lib.ptr(grad_f), _lib.ptr(work), hi, lo,
            flags, _stream()))

    def born_call(plan, coef, dmat_p, df_d, geo, snap, drec, work, nt):
        fn = getattr(_lib.load(), "mifwi_%s_born" % prefix)
        _lib.check(fn(plan.handle, coef[0], _lib.ptr(dmat_p), *coef[1:], _lib.ptr(df_d), *geo, _lib.ptr(snap), 0,
                      *_three(drec), _lib.ptr(work), 0, nt, _lib.ZERO_STATE, _stream()))

    return tuple(staticmethod(fn) for fn in (forward_call, adjoint_call, born_call))


_forward_call, _adjoint_call, _born_call = (fn.__func__ for fn in _calls("fluid"))      # the tools time them directly

class _Fluid(Physics):
    """The three-field scheme as :class:`_driver.Propagate` and :func:`_driver.linearised` see it.  opts: pml_width,
    shots_per_group, free_surface, source_type, fd_order (the plan's) and record_pressure."""
    name = "fluid"
    rule = "elastic"
    model = "mat"
    grad_planes = moment_planes = (3,)
    not_served = "Born modelling across time checkpoints is not served"
    weight_returns = "%(n)d tensors of the shape of its arguments"
    forward_call, adjoint_call, born_call = _calls("fluid")
    inputs = staticmethod(lambda mat, pz, px, gp, o: elastic._padded_inputs(mat, pz, px, gp))
    traces = staticmethod(lambda o: 3 if o["record_pressure"] else 2)

    @staticmethod
    def plan(dims, device_index, o):
        return FluidPlan(*dims, o["pml_width"], device_index, o["shots_per_group"], o["free_surface"], o["source_type"],
                         o["fd_order"])


def _options(pml_width, shots_per_group, free_surface, source_type, fd_order, record_pressure):
    return dict(pml_width=int(pml_width), shots_per_group=int(shots_per_group), free_surface=1 if free_surface else 0,
                source_type=elastic.source_type_code(source_type), fd_order=int(fd_order),
                record_pressure=bool(record_pressure))


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
    opts = _options(pml_width, shots_per_group, free_surface, source_type, fd_order, record_pressure)
    if pseudo_hessian is not None and not isinstance(pseudo_hessian, PseudoHessian):
        raise MifwiError("pseudo_hessian must be a fluid.PseudoHessian holder or None")
    return Propagate.apply(mat, f, _Fluid, pz, px, geom, int(snapshot_budget), pseudo_hessian, opts)


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
    """born / gauss_newton_product through :func:`_driver.linearised`.  Returns (background traces, perturbed traces,
    hv): lists of 2 or 3 tensors."""
    _require_cuda(mat, "mat")
    opts = _options(pml_width, 0, free_surface, source_type, fd_order, record_pressure)
    if mat.dim() != 3 or mat.shape[0] != 3:
        raise MifwiError("mat must be [3, nz, nx] (fluid.materials)")
    if tuple(dmat.shape) != tuple(mat.shape):
        raise MifwiError("dmat must have the shape of mat, %s (got %s)" % (tuple(mat.shape), tuple(dmat.shape)))
    _require_cuda(dmat, "dmat")
    return linearised(_Fluid, name, mat, dmat, f, df, pz, px, (src_cell, src_w, rec_cell, rec_w), snapshot_budget, adjoint,
                      weight, opts)


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
