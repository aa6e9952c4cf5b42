"""Host side of the viscoelastic P-SV propagator (one relaxation mechanism of a generalised standard linear solid): the
eight material planes of a (vp, vs, rho, qp, qs) model, plan and buffer handling and the ``torch.autograd.Function``
around the HIP forward / adjoint / Born entry points ``mifwi_visco_*`` of csrc/mifwi_elastic.hip.

Serves pyapi_denise runs with ``PHYSICS = 1`` and ``L = 1``: field data whose amplitudes cannot be matched without
attenuation.  The scheme is :mod:`elastic`'s with three memory variables per shot (rxx, rzz on the sxx node, rxz on the sxz
node) and three more material planes; grid, C-PML tables, free surface, sources, receivers and snapshot planes are the
elastic ones, and so are the seismograms, bit for bit, where planes 5-7 are zero.  One launch per half step (no
single-launch loop, no fused V+S step, f32 snapshot planes, no pressure receivers).  All wave arithmetic is in libmifwi.so;
there is no CPU path.
"""
import math

import numpy as np
import torch

from . import _lib, _psv, elastic
from ._lib import MifwiError
from ._driver import _Geometry, _Plan, Propagate
from .elastic import DEFAULT_SNAPSHOT_BUDGET, SOURCE_TYPES  # noqa: F401


def relaxation(f_relax, dt):
    """``(a, b)`` of the memory-variable update ``r <- a r - b q``: with eta = dt / tau_sigma = 2 pi f_relax dt,
    ``a = (2 - eta) / (2 + eta)`` and ``b = 2 eta / (2 + eta)`` (Crank-Nicolson in time), in double."""
    f_relax, dt = float(f_relax), float(dt)
    if not (f_relax > 0.0 and math.isfinite(f_relax)):
        raise MifwiError("visco: f_relax must be positive and finite (got %r)" % f_relax)
    eta = 2.0 * math.pi * f_relax * dt
    if not 0.0 < eta < 2.0:
        raise MifwiError("visco: eta = 2 pi f_relax dt = %g must lie inside (0, 2): the relaxation time 1 / (2 pi f_relax) "
                         "is not resolved by dt" % eta)
    return (2.0 - eta) / (2.0 + eta), 2.0 * eta / (2.0 + eta)


def _dispersion(f_ref, f_relax):
    """s = (w tau_sigma)^2 / (1 + (w tau_sigma)^2) at w = 2 pi f_ref: the share of tau that acts at the reference frequency."""
    f_ref, f_relax = float(f_ref), float(f_relax)
    if not (f_relax > 0.0 and math.isfinite(f_relax)):
        raise MifwiError("visco: f_relax must be positive and finite (got %r)" % f_relax)
    if not (f_ref > 0.0 and math.isfinite(f_ref)):
        raise MifwiError("visco: f_ref must be positive and finite (got %r)" % f_ref)
    x = (f_ref / f_relax) ** 2
    return x / (1.0 + x)


def _check_q(qp, qs):
    for name, q in (("qp", qp), ("qs", qs)):
        bad = ~(q.detach() > 0)           # catches <= 0 and NaN; inf is allowed (no attenuation)
        if bool(bad.any()):
            raise MifwiError("visco.materials: %s must be positive (inf: lossless); %d cells are not" % (name, int(bad.sum())))


def _sh(a, dz, dx):
    a = torch.cat([a, a[-1:, :]], 0)[dz:dz + a.shape[0]] if dz else a
    a = torch.cat([a, a[:, -1:]], 1)[:, dx:dx + a.shape[1]] if dx else a
    return a


def _moduli(vp, vs, rho, qp, qs, sdisp, s, free_surface):
    """Planes 0, 1, 2, 5, 6, 7 of :func:`materials` (times s = dt/h)."""
    taup, taus = 2.0 / qp, 2.0 / qs
    pi_r = rho * vp * vp / (1.0 + sdisp * taup)
    mu_r = rho * vs * vs / (1.0 + sdisp * taus)
    mu_u = mu_r * (1.0 + taus)
    lam_u = pi_r * (1.0 + taup) - 2.0 * mu_u
    # sxz node: harmonic mu_r (zero where a corner is zero) as elastic.staggered_materials, arithmetic tau_s
    m4 = [mu_r, _sh(mu_r, 0, 1), _sh(mu_r, 1, 0), _sh(mu_r, 1, 1)]
    anyzero = (m4[0] == 0) | (m4[1] == 0) | (m4[2] == 0) | (m4[3] == 0)
    inv = sum(1.0 / torch.where(m == 0, torch.ones_like(m), m) for m in m4)
    mur_xz = torch.where(anyzero, torch.zeros_like(mu_r), 4.0 / inv)
    taus_xz = 0.25 * (taus + _sh(taus, 0, 1) + _sh(taus, 1, 0) + _sh(taus, 1, 1))
    Ls, Ms = lam_u * s, (lam_u + 2.0 * mu_u) * s
    R1 = pi_r * taup * s
    R2 = (pi_r * taup - 2.0 * (mu_r * taus)) * s
    if free_surface:
        top = torch.zeros_like(Ls)
        top[0] = 1.0
        R1 = R1 - top * (R2 * Ls / Ms)
        R2 = R2 * (1.0 - top)
        Ms = Ms - top * (Ls * Ls / Ms)
        Ls = Ls * (1.0 - top)
    return Ls, Ms, mur_xz * (1.0 + taus_xz) * s, R2, R1, mur_xz * taus_xz * s


def materials(vp, vs, rho, qp, qs, f_ref, f_relax, dt, h, free_surface=False):
    """[8, nz, nx] = lam_u, lam2mu_u, mu_u_xz, dt/(h rho_x), dt/(h rho_z), R2, R1, rmu_xz, the moduli times dt/h, of a
    one-mechanism standard linear solid with quality factors ``qp``, ``qs`` (``inf``: lossless) whose phase velocities AT
    ``f_ref`` are ``vp`` and ``vs`` (DENISE's convention) and whose relaxation frequency is ``f_relax``.

    With tau_p = 2 / qp, tau_s = 2 / qs, tau_sigma = 1 / (2 pi f_relax) and s = (2 pi f_ref tau_sigma)^2 / (1 + (2 pi
    f_ref tau_sigma)^2): relaxed pi_r = rho vp^2 / (1 + s tau_p), mu_r = rho vs^2 / (1 + s tau_s); unrelaxed lam2mu_u =
    pi_r (1 + tau_p), mu_u = mu_r (1 + tau_s), lam_u their difference; R1 = pi_r tau_p, R2 = pi_r tau_p - 2 mu_r tau_s.  At
    the sxz node mu_r is averaged harmonically as ``elastic.staggered_materials`` averages mu (zero where any corner is
    zero) and tau_s arithmetically over the same four nodes: mu_u_xz = mu_r_xz (1 + tau_s_xz), rmu_xz = mu_r_xz tau_s_xz.
    Planes 3 and 4 are those of ``elastic.staggered_materials`` - the same bits.  Under ``free_surface`` row 0 is in the
    effective form of the stress-imaging condition (szz = 0 there): ``R1 -= R2 lam_u / lam2mu_u``, ``R2 = 0``,
    ``lam2mu_u -= lam_u^2 / lam2mu_u``, ``lam_u = 0`` with the row's earlier values on the right-hand sides (for the memory
    part an approximation, like DENISE's).  qp = qs = inf gives the elastic planes and zeros.

    A plain torch expression, differentiable w.r.t. all five planes, on any device and dtype (CPU float64 included): this
    form is the definition."""
    sdisp = _dispersion(f_ref, f_relax)
    relaxation(f_relax, dt)
    _check_q(qp, qs)
    Ls, Ms, mu_xz, R2, R1, rmu_xz = _moduli(vp, vs, rho, qp, qs, sdisp, dt / h, free_surface)
    m5 = elastic.staggered_materials(vp, vs, rho, dt, h)
    return torch.stack([Ls, Ms, mu_xz, m5[3], m5[4], R2, R1, rmu_xz])


def materials_jvp(vp, vs, rho, qp, qs, dvp, dvs, drho, dqp, dqs, f_ref, f_relax, dt, h, free_surface=False):
    """dmat [8, nz, nx]: the first-order change of :func:`materials` for the model perturbation - forward mode of the torch
    expression above for the six moduli; planes 3 and 4 through ``elastic.materials_jvp``.  Keep ``dvs`` = 0 where vs = 0
    and ``dqp`` = ``dqs`` = 0 where q = inf.  The transpose of the VJP autograd runs through :func:`materials`."""
    prm = [torch.as_tensor(t).detach() for t in (vp, vs, rho, qp, qs)]
    tan = [torch.as_tensor(t).detach().to(device=prm[0].device, dtype=prm[0].dtype) for t in (dvp, dvs, drho, dqp, dqs)]
    if any(t.shape != prm[0].shape for t in prm + tan) or prm[0].dim() != 2:
        raise MifwiError("materials_jvp: the five model planes and their perturbations must be [nz, nx] tensors of one shape")
    sdisp = _dispersion(f_ref, f_relax)
    relaxation(f_relax, dt)
    _check_q(prm[3], prm[4])
    d5 = elastic.materials_jvp(prm[0], prm[1], prm[2], tan[0], tan[1], tan[2], dt, h)
    d6 = torch.func.jvp(lambda *m: torch.stack(_moduli(*m, sdisp, dt / h, free_surface)), tuple(prm), tuple(tan))[1]
    return torch.stack([d6[0], d6[1], d6[2], d5[3], d5[4], d6[3], d6[4], d6[5]])


def max_velocity(vp, qp, f_ref, f_relax):
    """``max vp sqrt((1 + tau_p) / (1 + s tau_p))``: the unrelaxed (high-frequency) P velocity, the fastest the medium
    carries and the velocity :func:`profiles.elastic_cfl_limit` takes for a viscoelastic model."""
    sdisp = _dispersion(f_ref, f_relax)
    vp, qp = (torch.as_tensor(t if torch.is_tensor(t) else np.ascontiguousarray(t)).detach().to(torch.float64)
              for t in (vp, qp))
    taup = 2.0 / qp
    return float((vp * torch.sqrt((1.0 + taup) / (1.0 + sdisp * taup))).max())


class ViscoPlan(_Plan):
    PREFIX, LAYOUT = "visco", _lib.ViscoLayout

    def __init__(self, nz, nx, nt, nshot, nsrc, nrec, ntap, pml_width, device_index, relax_a, relax_b, shots_per_group=0,
                 free_surface=0, source_type=0, fd_order=4):
        self._create(_lib.ViscoDesc(nz, nx, nt, nshot, nsrc, nrec, ntap, pml_width, free_surface, shots_per_group,
                                    source_type, fd_order, relax_a, relax_b), device_index)


class _Visco(_psv.Psv, planes=8):
    """The viscoelastic scheme.  opts: pml_width, shots_per_group, free_surface, source_type, fd_order, relax_a, relax_b -
    the plan's."""
    name = "visco"
    mat_from = " (visco.materials)"
    Plan = ViscoPlan


def _options(pml_width, shots_per_group, free_surface, source_type, fd_order, f_relax, dt):
    a, b = relaxation(f_relax, dt)
    return dict(pml_width=int(pml_width), shots_per_group=int(shots_per_group), free_surface=1 if free_surface else 0,
                source_type=elastic.source_type_code(source_type), fd_order=int(fd_order), relax_a=a, relax_b=b)


def propagate(mat, f, pz, px, src_cell, src_w, rec_cell, rec_w, pml_width, f_relax, dt, shots_per_group=0,
              snapshot_budget=DEFAULT_SNAPSHOT_BUDGET, free_surface=False, source_type="explosive", fd_order=4,
              pseudo_hessian=None):
    """Viscoelastic forward modelling, differentiable w.r.t. ``mat`` and ``f``.

    mat [8,nz,nx] from :func:`materials` (built with the same ``f_relax`` and ``dt``);  f, pz, px, cells, taps,
    ``pml_width``, ``free_surface`` (build ``mat`` with it and ``pz`` with ``low=False``), ``source_type``, ``fd_order``,
    ``shots_per_group`` and ``snapshot_budget`` (time checkpointing when the snapshots do not fit; the checkpoints carry the
    memory variables) as in :func:`elastic.propagate`.  Returns (rec_vx, rec_vz), each [nt,nshot,nrec].  The gradient
    w.r.t. ``mat`` holds the elastic sums in planes 0-4 and, with w = -b (r_bar + sigma_bar / 2), g_R2 = sum (S1 wxx + S0
    wzz), g_R1 = sum (S0 wxx + S1 wzz), g_rmu = sum S2 wxz in planes 5-7.
    ``pseudo_hessian`` is refused: the viscoelastic parameter table of the pseudo-Hessian is not built.
    With ``mat[5:] == 0`` the seismograms are those of :func:`elastic.propagate` on ``mat[:5]`` (one launch per half step)
    bit for bit.  Repeated calls return the same bits under the conditions of :func:`elastic.propagate`."""
    _Visco.check_mat(mat)
    if pseudo_hessian is not None:
        raise MifwiError("visco.propagate: the pseudo-Hessian is not served for viscoelastic media (pseudo_hessian must be None)")
    opts = _options(pml_width, shots_per_group, free_surface, source_type, fd_order, f_relax, dt)
    geom = _Geometry.get(src_cell, src_w, rec_cell, rec_w, mat.device)
    f = f.to(device=mat.device)
    return Propagate.apply(mat, f, _Visco, pz, px, geom, int(snapshot_budget), None, opts)


def _linearised(name, mat, dmat, f, pz, px, src_cell, src_w, rec_cell, rec_w, pml_width, f_relax, dt, df, free_surface,
                fd_order, snapshot_budget, source_type, adjoint, weight):
    _Visco.check_mat(mat)
    opts = _options(pml_width, 0, free_surface, source_type, fd_order, f_relax, dt)
    return _psv.linearised(_Visco, name, mat, dmat, f, df, pz, px, (src_cell, src_w, rec_cell, rec_w), snapshot_budget,
                           adjoint, weight, opts)


def born(mat, dmat, f, pz, px, src_cell, src_w, rec_cell, rec_w, pml_width, f_relax, dt, df=None, free_surface=False,
         fd_order=4, snapshot_budget=DEFAULT_SNAPSHOT_BUDGET, source_type="explosive"):
    """Born / linearised modelling: returns ``(rec_vx, rec_vz, drec_vx, drec_vz)`` - the seismograms of the background
    ``mat`` (what :func:`propagate` returns, bit for bit) and ``drec = J (dmat, df)`` for the perturbation ``dmat``
    [8, nz, nx] of the material planes (:func:`materials_jvp`) and, optionally, ``df`` [nt, nshot, nsrc].  ``J`` is the exact
    transpose partner of the gradients autograd returns for :func:`propagate`.  No autograd through this call.  Shot chunks
    and refusals as :func:`elastic.born`; explosive sources only."""
    rec, drec, _ = _linearised("born", mat, dmat, f, pz, px, src_cell, src_w, rec_cell, rec_w, pml_width, f_relax, dt, df,
                               free_surface, fd_order, snapshot_budget, source_type, False, None)
    return tuple(rec) + tuple(drec)


def gauss_newton_product(mat, dmat, f, pz, px, src_cell, src_w, rec_cell, rec_w, pml_width, f_relax, dt, df=None,
                         free_surface=False, fd_order=4, snapshot_budget=DEFAULT_SNAPSHOT_BUDGET, weight=None,
                         source_type="explosive"):
    """Gauss-Newton Hessian-vector product ``hv = J^T W J dmat`` [8, nz, nx] with one background forward, one Born pass and
    one adjoint pass over the same resident snapshot buffer.  Returns ``(hv, drec_vx, drec_vz)``; ``weight`` and the shot
    chunks as in :func:`elastic.gauss_newton_product`."""
    _, drec, hv = _linearised("gauss_newton_product", mat, dmat, f, pz, px, src_cell, src_w, rec_cell, rec_w, pml_width,
                              f_relax, dt, df, free_surface, fd_order, snapshot_budget, source_type, True, weight)
    return (hv,) + tuple(drec)
