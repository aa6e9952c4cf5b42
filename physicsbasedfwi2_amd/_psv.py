"""What the four P-SV propagators (:mod:`elastic`, :mod:`vti`, :mod:`tti`, :mod:`visco`) share on the host: they are one scheme on one
plan of csrc/mifwi_elastic.hip - the medium decides the number of material planes and the names of the C entry points -
so they are one :class:`_driver.Physics` description, one set of calls into libmifwi.so and one set of argument checks.
A module keeps its material maps, its plan class, its options and its public functions; a further medium adds those and a
few lines over :class:`Psv`.
"""
import torch

from . import _driver, _lib
from ._lib import MifwiError
from ._driver import _require_cuda, _stream, Physics, pad_columns


def _padded_inputs(mat, pz, px, gp):
    """The material planes and C-PML tables as the C calls take them: on mat's device, rows padded to gp columns
    (materials and a, b 0, 1/kappa - rows 2 and 5 of the table - 1 there)."""
    dev = mat.device
    px_p = pad_columns(px.to(device=dev, dtype=torch.float32), gp)
    px_p[2::3, mat.shape[2]:] = 1.0
    return pad_columns(mat, gp), pz.to(device=dev, dtype=torch.float32).contiguous(), px_p


def _entry(phys, call):
    return getattr(_lib.load(), "mifwi_%s_%s" % (phys.name, call))


def _forward_call(phys, plan, coef, f_d, geo, rec):
    """``forward(snap_ptr, work_ptr, b, e, flags)`` as the drivers take it; rec = [rec_vx, rec_vz, ...] (pressure traces
    are bound to the plan), or None: a re-run that samples nothing."""
    fn = _entry(phys, "forward")
    rvx, rvz = rec[:2] if rec else (None, None)
    args = (plan.handle, *coef, _lib.ptr(f_d), *geo, _lib.ptr(rvx), _lib.ptr(rvz))
    return lambda snap, work, b, e, flags: _lib.check(fn(*args, snap, work, b, e, flags, _stream()))


def _adjoint_call(phys, plan, coef, geo, g, grad_mat, grad_f, work):
    """``adjoint(snap_ptr, snap_first, hi, lo, flags)`` as the backward driver takes it; g = [g_vx, g_vz, ...]."""
    fn = _entry(phys, "backward")
    return lambda snap, first, hi, lo, flags: _lib.check(fn(
        plan.handle, *coef, *geo, _lib.ptr(g[0]), _lib.ptr(g[1]), snap, first, _lib.ptr(grad_mat), _lib.ptr(grad_f),
        _lib.ptr(work), hi, lo, flags, _stream()))


def _born_call(phys, plan, coef, dmat_p, df_d, geo, snap, drec, work, nt):
    _lib.check(_entry(phys, "born")(plan.handle, coef[0], _lib.ptr(dmat_p), *coef[1:], _lib.ptr(df_d), *geo, _lib.ptr(snap), 0,
                                    _lib.ptr(drec[0]), _lib.ptr(drec[1]), _lib.ptr(work), 0, nt, _lib.ZERO_STATE, _stream()))


def _check_mat(phys, mat):
    _require_cuda(mat, "mat")
    if mat.dim() != 3 or mat.shape[0] != phys.grad_planes[0]:
        raise MifwiError("mat must be [%d, nz, nx]%s" % (phys.grad_planes[0], phys.mat_from))


class Psv(Physics):
    """A medium on the elastic plan as :class:`_driver.Propagate` and :func:`_driver.linearised` see it:
    ``class _Vti(Psv, planes=6)`` with ``name`` (the ``mifwi_<name>_*`` entry points), ``Plan`` and ``mat_from``."""
    rule = "elastic"
    model = "mat"
    not_served = "Born modelling across time checkpoints is not served"
    weight_returns = "(g_vx, g_vz) of the shape of its arguments"
    mat_from = ""               # ends the refusal of a mat of another shape: where its planes come from
    # what born / gauss_newton_product (%s) refuse beyond a wrong shape
    linearised_serves = "%s serves explosive sources only (a force source needs df from the density at the source node)"
    forward_call, adjoint_call, born_call, check_mat = (classmethod(fn) for fn in
                                                        (_forward_call, _adjoint_call, _born_call, _check_mat))
    inputs = staticmethod(lambda mat, pz, px, gp, o: _padded_inputs(mat, pz, px, gp))
    traces = staticmethod(lambda o: 2)

    def __init_subclass__(cls, planes, **kw):
        super().__init_subclass__(**kw)
        cls.grad_planes = (planes,)

    @staticmethod
    def adjoint_sources(plan, g, shape, dev, o):
        return [torch.zeros(shape, device=dev) if t is None else t.to(dtype=torch.float32).contiguous() for t in g[:2]]


def linearised(phys, name, mat, dmat, f, df, pz, px, taps, snapshot_budget, adjoint, weight, opts):
    """born / gauss_newton_product (``name``) of a P-SV module: the argument checks they share, then
    :func:`_driver.linearised` over resident f32 snapshots.  Returns (background traces, perturbed traces, hv)."""
    if opts["source_type"] != 0 or opts.get("record_pressure"):
        raise MifwiError(phys.linearised_serves % name)
    phys.check_mat(mat)
    if tuple(dmat.shape) != tuple(mat.shape):
        raise MifwiError("dmat must have the shape of mat, %s (got %s)" % (tuple(mat.shape), tuple(dmat.shape)))
    _require_cuda(dmat, "dmat")
    return _driver.linearised(phys, name, mat, dmat, f, df, pz, px, taps, snapshot_budget, adjoint, weight, opts)
