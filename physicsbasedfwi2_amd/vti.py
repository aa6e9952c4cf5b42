"""Host side of the elastic P-SV propagator in a medium with vertical transverse isotropy (VTI): the six material planes
of a Thomsen model, plan and buffer handling and the ``torch.autograd.Function`` around the HIP forward / adjoint / Born
entry points ``mifwi_vti_*`` of csrc/mifwi_elastic.hip.

Serves pyapi_denise runs with ``PHYSICS = 3`` (this library's number for the P-SV VTI medium): marine field data whose
far offsets cannot be fitted kinematically without epsilon and delta.  The scheme is :mod:`elastic`'s with the stiffnesses
c11, c13, c33 on the sxx / szz node and c44 on the sxz node - one more material plane; grid, C-PML tables, free surface,
sources, receivers and snapshot planes are the elastic ones, and so are the seismograms, bit for bit, where c33 == c11.
One launch per half step (no single-launch loop, no fused V+S step, f32 snapshot planes, no pressure receivers).  All wave
arithmetic is in libmifwi.so; there is no CPU path.
"""
import numpy as np
import torch

from . import _lib, _psv, elastic
from ._lib import MifwiError
from ._driver import _Geometry, _Plan, Propagate
from .elastic import DEFAULT_SNAPSHOT_BUDGET, SOURCE_TYPES  # noqa: F401


def materials(vp0, vs0, rho, epsilon, delta, dt, h, free_surface=False):
    """[6, nz, nx] = c13, c11, c44_xz, dt/(h rho_x), dt/(h rho_z), c33, the stiffnesses times dt/h, of the Thomsen model
    (vertical velocities ``vp0``, ``vs0``, density, epsilon, delta).

    Planes 2, 3 and 4 are those of ``elastic.staggered_materials(vp0, vs0, rho, ...)`` - the same bits (harmonic c44 at
    the sxz node, arithmetic densities).  With the collocated ``c33 = rho vp0^2 dt/h`` and ``c44 = rho vs0^2 dt/h``:
    ``c11 = (1 + 2 epsilon) c33`` and ``c13 = sqrt((c33 - c44) ((1 + 2 delta) c33 - c44)) - c44`` (Thomsen 1986).  Under
    ``free_surface`` row 0 is in the effective form of the stress-imaging condition (szz = 0 there): ``c13 = 0`` and
    ``c11 -= c13^2 / c33``.  epsilon = delta = 0 gives lambda, lambda + 2 mu and lambda + 2 mu again: the isotropic planes
    up to the rounding of the square root.

    A plain torch expression, differentiable w.r.t. all five inputs, on any device and dtype (CPU float64 included): this
    form is the definition.  Raises where the radicand is negative (no real c13: exactly one of ``vp0 > vs0`` and
    ``(1 + 2 delta) vp0^2 > vs0^2`` holds)."""
    c13, c11, c33 = _stiffnesses(vp0, vs0, rho, epsilon, delta, dt / h, free_surface, check=True)
    m5 = elastic.staggered_materials(vp0, vs0, rho, dt, h)
    return torch.stack([c13, c11, m5[2], m5[3], m5[4], c33])


def _stiffnesses(vp0, vs0, rho, epsilon, delta, s, free_surface, check):
    """(c13, c11, c33) times s = dt/h of :func:`materials`."""
    c33 = rho * vp0 * vp0 * s
    c44 = rho * vs0 * vs0 * s
    rad = (c33 - c44) * ((1.0 + 2.0 * delta) * c33 - c44)
    if check and bool((rad.detach() < 0).any()):
        raise MifwiError("vti.materials: (c33 - c44) ((1 + 2 delta) c33 - c44) is negative in %d cells: no real c13 "
                         "(delta too negative for this vs0 / vp0, or vs0 above vp0)" % int((rad.detach() < 0).sum()))
    c13 = torch.sqrt(rad) - c44
    c11 = (1.0 + 2.0 * epsilon) * c33
    if free_surface:
        top = torch.zeros_like(c33)
        top[0] = 1.0
        c11 = c11 - top * (c13 * c13 / c33)
        c13 = c13 * (1.0 - top)
    return c13, c11, c33


def materials_jvp(vp0, vs0, rho, epsilon, delta, dvp0, dvs0, drho, depsilon, ddelta, dt, h, free_surface=False):
    """dmat [6, nz, nx]: the first-order change of :func:`materials` for the model perturbation - forward mode of the
    torch expression above for planes 0, 1 and 5; planes 2-4 through ``elastic.materials_jvp`` (finite where vs0 = 0;
    keep ``dvs0`` = 0 there).  The transpose of the VJP autograd runs through :func:`materials`."""
    prm = [torch.as_tensor(t).detach() for t in (vp0, vs0, rho, epsilon, delta)]
    tan = [torch.as_tensor(t).detach().to(device=prm[0].device, dtype=prm[0].dtype)
           for t in (dvp0, dvs0, drho, depsilon, ddelta)]
    if any(t.shape != prm[0].shape for t in prm + tan) or prm[0].dim() != 2:
        raise MifwiError("materials_jvp: the five model planes and their perturbations must be [nz, nx] tensors of one shape")
    d5 = elastic.materials_jvp(prm[0], prm[1], prm[2], tan[0], tan[1], tan[2], dt, h)

    _stiffnesses(*prm, dt / h, free_surface, check=True)
    d3 = torch.func.jvp(lambda *m: torch.stack(_stiffnesses(*m, dt / h, free_surface, check=False)), tuple(prm), tuple(tan))[1]
    return torch.stack([d3[0], d3[1], d5[2], d5[3], d5[4], d3[2]])


def max_velocity(vp0, epsilon, delta):
    """``max vp0 sqrt(1 + 2 max(epsilon, delta, 0))``: an upper bound of the qP phase velocity over all angles, the
    velocity :func:`profiles.elastic_cfl_limit` takes for a VTI model."""
    vp0, epsilon, delta = (torch.as_tensor(t if torch.is_tensor(t) else np.ascontiguousarray(t)).detach().to(torch.float64)
                           for t in (vp0, epsilon, delta))
    a = torch.maximum(torch.maximum(epsilon, delta), torch.zeros_like(epsilon))
    return float((vp0 * torch.sqrt(1.0 + 2.0 * a)).max())


class VtiPlan(_Plan):
    PREFIX, LAYOUT = "vti", _lib.VtiLayout

    def __init__(self, nz, nx, nt, nshot, nsrc, nrec, ntap, pml_width, device_index, shots_per_group=0, free_surface=0,
                 source_type=0, fd_order=4):
        self._create(_lib.VtiDesc(nz, nx, nt, nshot, nsrc, nrec, ntap, pml_width, free_surface, shots_per_group,
                                  source_type, fd_order), device_index)


class _Vti(_psv.Psv, planes=6):
    """The VTI scheme.  opts: pml_width, shots_per_group, free_surface, source_type, fd_order - the plan's."""
    name = "vti"
    mat_from = " (vti.materials)"
    Plan = VtiPlan


def _options(pml_width, shots_per_group, free_surface, source_type, fd_order):
    return dict(pml_width=int(pml_width), shots_per_group=int(shots_per_group), free_surface=1 if free_surface else 0,
                source_type=elastic.source_type_code(source_type), fd_order=int(fd_order))


def propagate(mat, f, pz, px, src_cell, src_w, rec_cell, rec_w, pml_width, shots_per_group=0,
              snapshot_budget=DEFAULT_SNAPSHOT_BUDGET, free_surface=False, source_type="explosive", fd_order=4,
              pseudo_hessian=None):
    """Elastic forward modelling in a VTI medium, differentiable w.r.t. ``mat`` and ``f``.

    mat [6,nz,nx] from :func:`materials`;  f, pz, px, cells, taps, ``pml_width``, ``free_surface`` (build ``mat`` with it
    and ``pz`` with ``low=False``), ``source_type``, ``fd_order``, ``shots_per_group`` and ``snapshot_budget`` (time
    checkpointing when the snapshots do not fit) as in :func:`elastic.propagate`.  Returns (rec_vx, rec_vz), each
    [nt,nshot,nrec].  The gradient w.r.t. ``mat`` holds, per plane: g_c13 = sum (sxx_bar S1 + szz_bar S0), g_c11 =
    sum sxx_bar S0, g_c44, g_bx, g_bz as the elastic planes 2-4, g_c33 = sum szz_bar S1.
    ``pseudo_hessian`` is refused: the VTI parameter table of the pseudo-Hessian is not built.
    With ``mat[5] == mat[1]`` the seismograms are those of :func:`elastic.propagate` on ``mat[:5]`` bit for bit.  Repeated
    calls return the same bits under the conditions of :func:`elastic.propagate`."""
    _Vti.check_mat(mat)
    if pseudo_hessian is not None:
        raise MifwiError("vti.propagate: the pseudo-Hessian is not served for VTI media (pseudo_hessian must be None)")
    geom = _Geometry.get(src_cell, src_w, rec_cell, rec_w, mat.device)
    f = f.to(device=mat.device)
    opts = _options(pml_width, shots_per_group, free_surface, source_type, fd_order)
    return Propagate.apply(mat, f, _Vti, pz, px, geom, int(snapshot_budget), None, opts)


def _linearised(name, mat, dmat, f, pz, px, src_cell, src_w, rec_cell, rec_w, pml_width, df, free_surface, fd_order,
                snapshot_budget, source_type, adjoint, weight):
    _Vti.check_mat(mat)
    opts = _options(pml_width, 0, free_surface, source_type, fd_order)
    return _psv.linearised(_Vti, name, mat, dmat, f, df, pz, px, (src_cell, src_w, rec_cell, rec_w), snapshot_budget,
                           adjoint, weight, opts)


def born(mat, dmat, f, pz, px, src_cell, src_w, rec_cell, rec_w, pml_width, df=None, free_surface=False, fd_order=4,
         snapshot_budget=DEFAULT_SNAPSHOT_BUDGET, source_type="explosive"):
    """Born / linearised modelling: returns ``(rec_vx, rec_vz, drec_vx, drec_vz)`` - the seismograms of the background
    ``mat`` (what :func:`propagate` returns, bit for bit) and ``drec = J (dmat, df)`` for the perturbation ``dmat``
    [6, nz, nx] of the material planes (:func:`materials_jvp`) and, optionally, ``df`` [nt, nshot, nsrc].  ``J`` is the exact
    transpose partner of the gradients autograd returns for :func:`propagate`.  No autograd through this call.  Shot chunks
    and refusals as :func:`elastic.born`; explosive sources only."""
    rec, drec, _ = _linearised("born", mat, dmat, f, pz, px, src_cell, src_w, rec_cell, rec_w, pml_width, df, free_surface,
                               fd_order, snapshot_budget, source_type, False, None)
    return tuple(rec) + tuple(drec)


def gauss_newton_product(mat, dmat, f, pz, px, src_cell, src_w, rec_cell, rec_w, pml_width, df=None, free_surface=False,
                         fd_order=4, snapshot_budget=DEFAULT_SNAPSHOT_BUDGET, weight=None, source_type="explosive"):
    """Gauss-Newton Hessian-vector product ``hv = J^T W J dmat`` [6, nz, nx] with one background forward, one Born pass and
    one adjoint pass over the same resident snapshot buffer.  Returns ``(hv, drec_vx, drec_vz)``; ``weight`` and the shot
    chunks as in :func:`elastic.gauss_newton_product`."""
    _, drec, hv = _linearised("gauss_newton_product", mat, dmat, f, pz, px, src_cell, src_w, rec_cell, rec_w, pml_width,
                              df, free_surface, fd_order, snapshot_budget, source_type, True, weight)
    return (hv,) + tuple(drec)
