"""Host side of the elastic P-SV propagator in a medium with a tilted symmetry axis (TTI): the eight material planes of a
Thomsen model with a tilt field, plan and buffer handling and the ``torch.autograd.Function`` around the HIP forward /
adjoint / Born entry points ``mifwi_tti_*`` of csrc/mifwi_elastic.hip (kernels in csrc/mifwi_tti.h).

Serves pyapi_denise runs with ``PHYSICS = 4`` (this library's number for the P-SV TTI medium): anisotropic data over
dipping beds - folded sediments, salt flanks - where the symmetry axis follows the bedding and a VTI inversion would map
the tilt into epsilon, delta and structure.  The scheme is :mod:`vti`'s with the stiffnesses rotated by the tilt, which
adds c15 and c35 on the sxx / szz node: the normal stresses feel the shear strain and the shear stress the normal strains,
through four-point averages between the two kinds of node and a 0/1 mask that switches the coupling off where the
harmonic c55 is 0 (include/mifwi.h has the scheme).  Grid, C-PML tables, free surface, sources, receivers and snapshot
planes are the elastic ones, and so are the seismograms of :mod:`vti`, bit for bit, where c15 = c35 = 0.  The stress half
step and its transpose are two launches each (no single-launch loop, no fused V+S step, f32 snapshot planes, no pressure
receivers).  All wave arithmetic is in libmifwi.so; there is no CPU path.
"""
import torch

from . import _lib, _psv, elastic, vti
from ._lib import MifwiError
from ._driver import _Geometry, _Plan, Propagate
from .elastic import DEFAULT_SNAPSHOT_BUDGET, SOURCE_TYPES  # noqa: F401
from .vti import max_velocity  # noqa: F401  (a rotation changes no phase velocity)


def materials(vp0, vs0, rho, epsilon, delta, theta, dt, h, free_surface=False):
    """[8, nz, nx] = c13, c11, c55_xz, dt/(h rho_x), dt/(h rho_z), c33, c15, c35, the stiffnesses times dt/h, of the Thomsen
    model (velocities ``vp0``, ``vs0`` along the symmetry axis, density, epsilon, delta) whose symmetry axis is tilted by
    ``theta`` (radians): for theta > 0 it points along (sin theta, cos theta) in (x, z), z down.

    The collocated VTI stiffnesses c33 = rho vp0^2, c44 = rho vs0^2, c11, c13 of :func:`vti.materials` are rotated, with
    c = cos theta and s = sin theta::

        c11' = c11 c^4 + c33 s^4 + 2 (c13 + 2 c44) s^2 c^2        c33' = c11 s^4 + c33 c^4 + 2 (c13 + 2 c44) s^2 c^2
        c13' = (c11 + c33 - 4 c44) s^2 c^2 + c13 (s^4 + c^4)      c55' = (c11 + c33 - 2 c13) s^2 c^2 + c44 (c^2 - s^2)^2
        c15' = (c13 - c11 + 2 c44) s c^3 - (c13 - c33 + 2 c44) s^3 c
        c35' = (c13 - c11 + 2 c44) s^3 c - (c13 - c33 + 2 c44) s c^3

    c55_xz is the harmonic four-point average of c55' (the rule of ``elastic.staggered_materials``: 0 where any of the four
    is 0, edges replicated); planes 3 and 4 are those of ``elastic.staggered_materials``; c15 and c35 sit on the sxx node.
    theta = 0 gives the six planes of :func:`vti.materials` bit for bit and c15 = c35 = 0 exactly; in water (vs0 = epsilon =
    delta = 0) c15, c35 and c55_xz are exactly 0 at any theta.  Under ``free_surface`` row 0 is kept VTI-like - the
    library's definition, there is no tilted surface row: c13 = c15 = c35 = 0 and c11 -= c13^2 / c33 there (in marine data
    that row is water, where all three vanish anyway).

    A plain torch expression, differentiable w.r.t. all six inputs, on any device and dtype (CPU float64 included): this
    form is the definition.  Raises where :func:`vti.materials` does (no real c13)."""
    c13, c11, c33, c55, c15, c35 = _stiffnesses(vp0, vs0, rho, epsilon, delta, theta, dt / h, free_surface, check=True)
    m5 = elastic.staggered_materials(vp0, vs0, rho, dt, h)
    return torch.stack([c13, c11, c55, m5[3], m5[4], c33, c15, c35])


def _rotated(vp0, vs0, rho, epsilon, delta, theta, s, check):
    """(c13', c11', c33', c55', c15', c35') times s: the collocated VTI stiffnesses of ``vti._stiffnesses`` rotated by
    theta.  At theta = 0 (cos = 1, sin = 0 exactly) every product with s^2 is an exact 0: the VTI bits."""
    c13, c11, c33 = vti._stiffnesses(vp0, vs0, rho, epsilon, delta, s, False, check)
    c44 = rho * vs0 * vs0 * s
    theta = torch.as_tensor(theta, dtype=c33.dtype, device=c33.device)
    co, si = torch.cos(theta), torch.sin(theta)
    c2, s2 = co * co, si * si
    c4, s4, s2c2 = c2 * c2, s2 * s2, s2 * c2
    mix = 2.0 * (c13 + 2.0 * c44) * s2c2
    r11 = c11 * c4 + c33 * s4 + mix
    r33 = c11 * s4 + c33 * c4 + mix
    r13 = (c11 + c33 - 4.0 * c44) * s2c2 + c13 * (s4 + c4)
    r55 = (c11 + c33 - 2.0 * c13) * s2c2 + c44 * ((c2 - s2) * (c2 - s2))
    a, b = c13 - c11 + 2.0 * c44, c13 - c33 + 2.0 * c44
    r15 = a * (si * c2 * co) - b * (s2 * si * co)
    r35 = a * (s2 * si * co) - b * (si * c2 * co)
    return r13, r11, r33, r55, r15, r35


def _stiffnesses(vp0, vs0, rho, epsilon, delta, theta, s, free_surface, check):
    """(c13', c11', c33', c55_xz, c15', c35') of :func:`materials`: the rotated stiffnesses times s = dt/h, row 0 in the
    surface form under ``free_surface``; c55_xz is averaged before the scaling, as ``elastic.staggered_materials`` averages
    mu (the same bits at theta = 0)."""
    r13, r11, r33, _, r15, r35 = _rotated(vp0, vs0, rho, epsilon, delta, theta, s, check)
    r55 = _harmonic_xz(_rotated(vp0, vs0, rho, epsilon, delta, theta, 1.0, False)[3]) * s
    if free_surface:
        top = torch.zeros_like(r33)
        top[0] = 1.0
        r11 = r11 - top * (r13 * r13 / r33)
        r13, r15, r35 = r13 * (1.0 - top), r15 * (1.0 - top), r35 * (1.0 - top)
    return r13, r11, r33, r55, r15, r35


def _harmonic_xz(c):
    """The harmonic four-point average at the sxz node of ``elastic._staggered_materials_torch``: 0 where any of the four
    is 0, edges replicated."""
    nz, nx = c.shape
    zi = torch.arange(nz, device=c.device).clamp(max=nz - 2) + 1 if nz > 1 else torch.zeros(nz, dtype=torch.long, device=c.device)
    xi = torch.arange(nx, device=c.device).clamp(max=nx - 2) + 1 if nx > 1 else torch.zeros(nx, dtype=torch.long, device=c.device)
    four = (c, c[:, xi], c[zi], c[zi][:, xi])
    dead = (four[0] == 0) | (four[1] == 0) | (four[2] == 0) | (four[3] == 0)
    safe = [torch.where(dead, torch.ones_like(q), q) for q in four]
    return torch.where(dead, torch.zeros_like(c), 4.0 / (1.0 / safe[0] + 1.0 / safe[1] + 1.0 / safe[2] + 1.0 / safe[3]))


def materials_jvp(vp0, vs0, rho, epsilon, delta, theta, dvp0, dvs0, drho, depsilon, ddelta, dtheta, dt, h,
                  free_surface=False):
    """dmat [8, nz, nx]: the first-order change of :func:`materials` for the model perturbation - forward mode of the
    torch expression above; planes 3 and 4 through ``elastic.materials_jvp``.  Where c55_xz is 0 its change is 0 (the mask
    of the scheme is a constant); keep ``dvs0`` = 0 where vs0 = 0.  The transpose of the VJP autograd runs through
    :func:`materials`."""
    prm = [torch.as_tensor(t).detach() for t in (vp0, vs0, rho, epsilon, delta, theta)]
    tan = [torch.as_tensor(t).detach().to(device=prm[0].device, dtype=prm[0].dtype)
           for t in (dvp0, dvs0, drho, depsilon, ddelta, dtheta)]
    if any(t.shape != prm[0].shape for t in prm + tan) or prm[0].dim() != 2:
        raise MifwiError("materials_jvp: the six model planes and their perturbations must be [nz, nx] tensors of one shape")
    d5 = elastic.materials_jvp(prm[0], prm[1], prm[2], tan[0], tan[1], tan[2], dt, h)
    _stiffnesses(*prm, dt / h, free_surface, check=True)

    def six(*m):
        c13, c11, c33, c55, c15, c35 = _stiffnesses(*m, dt / h, free_surface, check=False)
        return torch.stack([c13, c11, c55, c33, c15, c35])
    d6 = torch.func.jvp(six, tuple(prm), tuple(tan))[1]
    return torch.stack([d6[0], d6[1], d6[2], d5[3], d5[4], d6[3], d6[4], d6[5]])


class TtiPlan(_Plan):
    PREFIX, LAYOUT = "tti", _lib.TtiLayout

    def __init__(self, nz, nx, nt, nshot, nsrc, nrec, ntap, pml_width, device_index, shots_per_group=0, free_surface=0,
                 source_type=0, fd_order=4):
        self._create(_lib.TtiDesc(nz, nx, nt, nshot, nsrc, nrec, ntap, pml_width, free_surface, shots_per_group,
                                  source_type, fd_order), device_index)


class _Tti(_psv.Psv, planes=8):
    """The TTI scheme.  opts: pml_width, shots_per_group, free_surface, source_type, fd_order - the plan's."""
    name = "tti"
    mat_from = " (tti.materials)"
    Plan = TtiPlan


_options = vti._options


def propagate(mat, f, pz, px, src_cell, src_w, rec_cell, rec_w, pml_width, shots_per_group=0,
              snapshot_budget=DEFAULT_SNAPSHOT_BUDGET, free_surface=False, source_type="explosive", fd_order=4,
              pseudo_hessian=None):
    """Elastic forward modelling in a TTI medium, differentiable w.r.t. ``mat`` and ``f``.

    mat [8,nz,nx] from :func:`materials`; every other argument as in :func:`vti.propagate`.  Returns (rec_vx, rec_vz), each
    [nt,nshot,nrec].  The gradient w.r.t. ``mat`` holds the six VTI planes' gradients and, with A the four-point average
    from sxz nodes to the sxx node and w the mask of the scheme, g_c15 = sum (sxx_bar A(w S2) + S0 A(w sxz_bar)) and
    g_c35 = sum (szz_bar A(w S2) + S1 A(w sxz_bar)).  ``pseudo_hessian`` is refused: the TTI parameter table of the
    pseudo-Hessian is not built.  With ``mat[6] == mat[7] == 0`` the seismograms are those of :func:`vti.propagate` on
    ``mat[:6]`` bit for bit.  Repeated calls return the same bits under the conditions of :func:`elastic.propagate`."""
    _Tti.check_mat(mat)
    if pseudo_hessian is not None:
        raise MifwiError("tti.propagate: the pseudo-Hessian is not served for TTI media (pseudo_hessian must be None)")
    geom = _Geometry.get(src_cell, src_w, rec_cell, rec_w, mat.device)
    f = f.to(device=mat.device)
    opts = _options(pml_width, shots_per_group, free_surface, source_type, fd_order)
    return Propagate.apply(mat, f, _Tti, pz, px, geom, int(snapshot_budget), None, opts)


def _linearised(name, mat, dmat, f, pz, px, src_cell, src_w, rec_cell, rec_w, pml_width, df, free_surface, fd_order,
                snapshot_budget, source_type, adjoint, weight):
    _Tti.check_mat(mat)
    opts = _options(pml_width, 0, free_surface, source_type, fd_order)
    return _psv.linearised(_Tti, name, mat, dmat, f, df, pz, px, (src_cell, src_w, rec_cell, rec_w), snapshot_budget,
                           adjoint, weight, opts)


def born(mat, dmat, f, pz, px, src_cell, src_w, rec_cell, rec_w, pml_width, df=None, free_surface=False, fd_order=4,
         snapshot_budget=DEFAULT_SNAPSHOT_BUDGET, source_type="explosive"):
    """Born / linearised modelling: returns ``(rec_vx, rec_vz, drec_vx, drec_vz)`` as :func:`vti.born`, for the
    perturbation ``dmat`` [8, nz, nx] of the material planes (:func:`materials_jvp`); the mask of the scheme comes from the
    background ``mat[2]``.  Explosive sources only."""
    rec, drec, _ = _linearised("born", mat, dmat, f, pz, px, src_cell, src_w, rec_cell, rec_w, pml_width, df, free_surface,
                               fd_order, snapshot_budget, source_type, False, None)
    return tuple(rec) + tuple(drec)


def gauss_newton_product(mat, dmat, f, pz, px, src_cell, src_w, rec_cell, rec_w, pml_width, df=None, free_surface=False,
                         fd_order=4, snapshot_budget=DEFAULT_SNAPSHOT_BUDGET, weight=None, source_type="explosive"):
    """Gauss-Newton Hessian-vector product ``hv = J^T W J dmat`` [8, nz, nx] as :func:`vti.gauss_newton_product`.  Returns
    ``(hv, drec_vx, drec_vz)``."""
    _, drec, hv = _linearised("gauss_newton_product", mat, dmat, f, pz, px, src_cell, src_w, rec_cell, rec_w, pml_width,
                              df, free_surface, fd_order, snapshot_budget, source_type, True, weight)
    return (hv,) + tuple(drec)
