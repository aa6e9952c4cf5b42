"""Host side of the viscoacoustic fluid propagator (one relaxation mechanism of a standard linear solid on the fluid
kernels): the four material planes of a (vp, rho, qp) model, plan and buffer handling and the
``torch.autograd.Function`` around the HIP forward / adjoint / Born entry points ``mifwi_viscofluid_*`` of
csrc/mifwi_fluid.hip.

Serves pyapi_denise runs with ``PHYSICS = 2``, ``acoustic_kernels = "fluid"`` and ``L = 1``: marine field data whose
amplitudes a lossless medium cannot match.  The scheme is :mod:`fluid`'s with one memory variable per shot (r on the p
node) and one more material plane; grid, C-PML tables, free surface, sources, receivers (pressure included) and snapshot
planes are the fluid ones, and so are the seismograms, bit for bit, where plane 3 is zero.  It is equally :mod:`visco`'s
with Vs = 0, on four fields instead of eight: ``rec_vx, rec_vz`` are its bits.  One launch per half step.  All wave
arithmetic is in libmifwi.so; there is no CPU path.
"""
import torch

from . import _lib, elastic, fluid, visco
from ._lib import MifwiError
from ._driver import _Geometry, _Plan, _require_cuda, Propagate, linearised
from .elastic import DEFAULT_SNAPSHOT_BUDGET, SOURCE_TYPES  # noqa: F401
from .fluid import force_amplitude  # noqa: F401  (planes 1 and 2 are the fluid's)
from .visco import max_velocity, relaxation  # noqa: F401  (the unrelaxed velocity; (a, b) of the memory update)


def _moduli(vp, rho, qp, sdisp, s, free_surface):
    """Planes 0 and 3 of :func:`materials` (times s = dt/h): ``visco._moduli`` with vs = 0, operation by operation."""
    taup = 2.0 / qp
    pi_r = rho * vp * vp / (1.0 + sdisp * taup)
    Ku = pi_r * (1.0 + taup) * s
    R = pi_r * taup * s
    if free_surface:
        keep = torch.ones_like(Ku)
        keep[0] = 0.0
        Ku, R = Ku * keep, R * keep
    return Ku, R


def _check_q(qp):
    bad = ~(qp.detach() > 0)           # catches <= 0 and NaN; inf is allowed (no attenuation)
    if bool(bad.any()):
        raise MifwiError("viscofluid.materials: qp must be positive (inf: lossless); %d cells are not" % int(bad.sum()))


def materials(vp, rho, qp, f_ref, f_relax, dt, h, free_surface=False):
    """[4, nz, nx] = K_u dt/h, dt/(h rho_x), dt/(h rho_z), R dt/h of a one-mechanism standard linear solid with quality
    factor ``qp`` (``inf``: lossless) whose phase velocity AT ``f_ref`` is ``vp`` (DENISE's convention) and whose relaxation
    frequency is ``f_relax``.

    With tau_p = 2 / qp and s as ``visco._dispersion(f_ref, f_relax)``: relaxed pi_r = rho vp^2 / (1 + s tau_p), unrelaxed
    K_u = pi_r (1 + tau_p), R = pi_r tau_p - planes 0 and 6 of ``visco.materials(vp, 0, rho, qp, inf, ...)`` away from a
    free-surface row.  Planes 1 and 2 are those of :func:`fluid.materials` - the same bits.  Under ``free_surface`` row 0 of
    planes 0 and 3 is 0 (p = 0 there).  ``qp = inf`` gives :func:`fluid.materials` and a zero plane.

    A plain torch expression, differentiable w.r.t. vp, rho and qp, on any device and dtype (CPU float64 included): this
    form is the definition."""
    sdisp = visco._dispersion(f_ref, f_relax)
    relaxation(f_relax, dt)
    _check_q(qp)
    Ku, R = _moduli(vp, rho, qp, sdisp, dt / h, free_surface)
    m5 = elastic.staggered_materials(vp, torch.zeros_like(vp), rho, dt, h)
    return torch.stack([Ku, m5[3], m5[4], R])


def materials_jvp(vp, rho, qp, dvp, drho, dqp, f_ref, f_relax, dt, h, free_surface=False):
    """dmat [4, nz, nx]: the first-order change of :func:`materials` for the model perturbation (dvp, drho, dqp) - forward
    mode of the torch expression above for planes 0 and 3; planes 1 and 2 through ``elastic.materials_jvp``.  Keep ``dqp`` =
    0 where qp = inf.  The transpose of the VJP autograd runs through :func:`materials`."""
    prm = [torch.as_tensor(t).detach() for t in (vp, rho, qp)]
    tan = [torch.as_tensor(t).detach().to(device=prm[0].device, dtype=prm[0].dtype) for t in (dvp, drho, dqp)]
    if any(t.shape != prm[0].shape for t in prm + tan) or prm[0].dim() != 2:
        raise MifwiError("materials_jvp: the three model planes and their perturbations must be [nz, nx] tensors of one shape")
    sdisp = visco._dispersion(f_ref, f_relax)
    relaxation(f_relax, dt)
    _check_q(prm[2])
    zero = torch.zeros_like(prm[0])
    d5 = elastic.materials_jvp(prm[0], zero, prm[1], tan[0], zero, tan[1], dt, h)
    d2 = torch.func.jvp(lambda *m: torch.stack(_moduli(*m, sdisp, dt / h, free_surface)), tuple(prm), tuple(tan))[1]
    return torch.stack([d2[0], d5[3], d5[4], d2[1]])


class ViscofluidPlan(_Plan):
    PREFIX, LAYOUT = "viscofluid", _lib.ViscofluidLayout

    def __init__(self, nz, nx, nt, nshot, nsrc, nrec, ntap, pml_width, device_index, relax_a, relax_b, shots_per_group=0,
                 free_surface=0, source_type=0, fd_order=4):
        self._create(_lib.ViscofluidDesc(nz, nx, nt, nshot, nsrc, nrec, ntap, pml_width, free_surface, shots_per_group,
                                         source_type, fd_order, relax_a, relax_b), device_index)


class _Viscofluid(fluid._Fluid):
    """The four-field scheme as :class:`_driver.Propagate` and :func:`_driver.linearised` see it.  opts: those of
    :class:`fluid._Fluid` and relax_a, relax_b."""
    name = "viscofluid"
    grad_planes = (4,)
    moment_planes = None           # no pseudo-Hessian: propagate refuses the holder
    forward_call, adjoint_call, born_call = fluid._calls("viscofluid")

    @staticmethod
    def plan(dims, device_index, o):
        return ViscofluidPlan(*dims, o["pml_width"], device_index, o["relax_a"], o["relax_b"], o["shots_per_group"],
                              o["free_surface"], o["source_type"], o["fd_order"])


def _options(pml_width, shots_per_group, free_surface, source_type, fd_order, record_pressure, f_relax, dt):
    a, b = relaxation(f_relax, dt)
    return dict(fluid._options(pml_width, shots_per_group, free_surface, source_type, fd_order, record_pressure),
                relax_a=a, relax_b=b)


def _check_mat(mat):
    _require_cuda(mat, "mat")
    if mat.dim() != 3 or mat.shape[0] != 4:
        raise MifwiError("mat must be [4, nz, nx] (viscofluid.materials)")


def propagate(mat, f, pz, px, src_cell, src_w, rec_cell, rec_w, pml_width, f_relax, dt, free_surface=False,
              source_type="explosive", record_pressure=False, fd_order=4, shots_per_group=0,
              snapshot_budget=DEFAULT_SNAPSHOT_BUDGET, pseudo_hessian=None):
    """Viscoacoustic forward modelling in a variable-density medium, differentiable w.r.t. ``mat`` and ``f``.

    mat [4,nz,nx] from :func:`materials` (built with the same ``f_relax`` and ``dt``); every other argument, the sources
    ("explosive" / "fx" / "fz", :func:`force_amplitude`), ``record_pressure`` and the returned (rec_vx, rec_vz[, rec_p]) as
    in :func:`fluid.propagate`; time checkpoints carry the memory variable.  The gradient w.r.t. ``mat`` holds the fluid
    sums in planes 0-2 and, with w = -b (r_bar + p_bar / 2), g_R = sum S0 w in plane 3.
    ``pseudo_hessian`` is refused: the viscoacoustic parameter table of the pseudo-Hessian is not built.
    With ``mat[3] == 0`` the seismograms are those of :func:`fluid.propagate` on ``mat[:3]`` bit for bit; on the planes of
    a model, rec_vx and rec_vz are those of :func:`visco.propagate` on ``visco.materials(vp, 0, rho, qp, inf, ...)`` (one
    launch per half step) bit for bit, within rounding of the surface row under ``free_surface``.  Repeated calls return
    the same bits under the conditions of :func:`fluid.propagate`."""
    _check_mat(mat)
    if pseudo_hessian is not None:
        raise MifwiError("viscofluid.propagate: the pseudo-Hessian is not served for viscoacoustic media (pseudo_hessian "
                         "must be None)")
    opts = _options(pml_width, shots_per_group, free_surface, source_type, fd_order, record_pressure, f_relax, dt)
    geom = _Geometry.get(src_cell, src_w, rec_cell, rec_w, mat.device)
    f = f.to(device=mat.device)
    return Propagate.apply(mat, f, _Viscofluid, pz, px, geom, int(snapshot_budget), None, opts)


def _linearised(name, mat, dmat, f, pz, px, src_cell, src_w, rec_cell, rec_w, pml_width, f_relax, dt, df, free_surface,
                source_type, record_pressure, fd_order, snapshot_budget, adjoint, weight):
    _check_mat(mat)
    opts = _options(pml_width, 0, free_surface, source_type, fd_order, record_pressure, f_relax, dt)
    if tuple(dmat.shape) != tuple(mat.shape):
        raise MifwiError("dmat must have the shape of mat, %s (got %s)" % (tuple(mat.shape), tuple(dmat.shape)))
    _require_cuda(dmat, "dmat")
    return linearised(_Viscofluid, name, mat, dmat, f, df, pz, px, (src_cell, src_w, rec_cell, rec_w), snapshot_budget,
                      adjoint, weight, opts)


def born(mat, dmat, f, pz, px, src_cell, src_w, rec_cell, rec_w, pml_width, f_relax, dt, df=None, free_surface=False,
         source_type="explosive", record_pressure=False, fd_order=4, snapshot_budget=DEFAULT_SNAPSHOT_BUDGET):
    """Born / linearised modelling: returns ``(rec_vx, rec_vz[, rec_p], drec_vx, drec_vz[, drec_p])`` - the seismograms of
    the background ``mat`` (what :func:`propagate` returns, bit for bit) and ``drec = J (dmat, df)`` for the perturbation
    ``dmat`` [4, nz, nx] of the material planes (:func:`materials_jvp`) and, optionally, ``df`` [nt, nshot, nsrc], injected
    where ``f`` is for every ``source_type``.  ``J`` is the exact transpose partner of the gradients autograd returns for
    :func:`propagate`.  No autograd through this call.  Shot chunks and refusals as :func:`fluid.born`."""
    rec, drec, _ = _linearised("born", mat, dmat, f, pz, px, src_cell, src_w, rec_cell, rec_w, pml_width, f_relax, dt, df,
                               free_surface, source_type, record_pressure, fd_order, snapshot_budget, False, None)
    return tuple(rec) + tuple(drec)


def gauss_newton_product(mat, dmat, f, pz, px, src_cell, src_w, rec_cell, rec_w, pml_width, f_relax, dt, df=None,
                         free_surface=False, source_type="explosive", record_pressure=False, fd_order=4,
                         snapshot_budget=DEFAULT_SNAPSHOT_BUDGET, weight=None):
    """Gauss-Newton Hessian-vector product ``hv = J^T W J dmat`` [4, nz, nx] with one background forward, one Born pass and
    one adjoint pass over the same resident snapshot buffer.  Returns ``(hv, drec_vx, drec_vz[, drec_p])``; ``weight`` and
    the shot chunks as in :func:`fluid.gauss_newton_product`."""
    _, drec, hv = _linearised("gauss_newton_product", mat, dmat, f, pz, px, src_cell, src_w, rec_cell, rec_w, pml_width,
                              f_relax, dt, df, free_surface, source_type, record_pressure, fd_order, snapshot_budget, True,
                              weight)
    return (hv,) + tuple(drec)
