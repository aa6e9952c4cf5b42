"""Host side of the elastic (P-SV) propagator: staggered material preparation (differentiable
torch ops, so the chain rule (vp, vs, rho) -> (lambda, mu, averages) is autograd's), plan and
buffer handling, and the ``torch.autograd.Function`` around the HIP forward / adjoint.

Stands where ``d.forward`` / ``d.grad`` of pyapi_denise stand in the reference
(models/networks.py:7752-7802): models in, vx/vz seismograms and Vp/Vs/rho gradients out,
with no mpirun and no files.  All wave arithmetic is in libmifwi.so; there is no CPU path.
"""
import os
import weakref

import torch

from . import _lib, _psv
from ._lib import MifwiError
from ._driver import _Geometry, _MomentsHolder, _Plan, _require_cuda, _stream, Physics, Propagate
from ._psv import _padded_inputs  # noqa: F401  (fluid.py and the rate tools take it from here)

# bytes of snapshot planes + time checkpoints a call may hold (288 GB of HBM per GPU; the rest is left to the caller's
# network and data); MIFWI_EL_SNAPSHOT_BUDGET_GB overrides it (measurements of the checkpointed path on short runs)
DEFAULT_SNAPSHOT_BUDGET = int(float(os.environ.get("MIFWI_EL_SNAPSHOT_BUDGET_GB", "96")) * (1 << 30))


SNAPSHOT_FORMATS = {"f32": _lib.SNAPSHOT_F32, "bf16": _lib.SNAPSHOT_BF16}
SOURCE_TYPES = {"explosive": 0, "fx": 1, "fz": 2, 0: 0, 1: 1, 2: 2}


def source_type_code(source_type):
    """"explosive" / "fx" / "fz" (or 0 / 1 / 2) -> the plans' source_type."""
    try:
        return SOURCE_TYPES[source_type]
    except KeyError:
        raise MifwiError("source_type must be one of %s" % sorted(k for k in SOURCE_TYPES if isinstance(k, str)))


def snapshot_mode():
    """Default storage of the five forward snapshot planes between the forward and the adjoint pass:
    "f32" (exact discrete adjoint) unless MIFWI_EL_SNAP=bf16 asks for the compressed planes (see
    :func:`propagate`, ``snapshot_format``)."""
    v = os.environ.get("MIFWI_EL_SNAP", "f32").lower()
    if v not in SNAPSHOT_FORMATS:
        raise MifwiError("MIFWI_EL_SNAP must be f32 or bf16 (got %r)" % v)
    return v


def snapshot_bytes_per_cell(fmt=None):
    return 10.0 if (fmt or snapshot_mode()) == "bf16" else 20.0


def kernel_family(flags):
    """(forward, adjoint) description of the formulation a plan picked (``plan.layout.kernel_flags``)."""
    fwd = ("single-launch time loop" if flags & _lib.EL_KERNEL_FWD_SINGLE_LAUNCH else
           "one fused V+S launch per step" if flags & _lib.EL_KERNEL_FWD_FUSED_STEP else "one launch per half step")
    adj = "single-launch time loop" if flags & _lib.EL_KERNEL_ADJ_SINGLE_LAUNCH else "one launch per half step"
    return fwd, adj


def other_per_step_env(flags=0):
    """(environment, label) selecting the other formulation of the per-step forward: bench.py's in-run
    cross-check runs one shot through both."""
    if flags & _lib.EL_KERNEL_FWD_FUSED_STEP:
        return {"MIFWI_EL_FUSED": "0"}, "one launch per half step"
    return {"MIFWI_EL_FUSED": "1"}, "fused V+S forward launch"


class _MaterialsFn(torch.autograd.Function):
    """staggered_materials on the device in ONE launch each way (csrc/mifwi_materials.hip): the torch expression below
    is ~60 elementwise launches forward and ~100 backward, 2 ms of a 46 ms gradient pass on the reference's 100x300 grid."""

    @staticmethod
    def forward(ctx, vp, vs, rho, s, free_surface):
        lib = _lib.load()
        dev = vp.device
        nz, nx = vp.shape
        ins = [t.detach().to(dtype=torch.float32).contiguous() for t in (vp, vs, rho)]
        out = torch.empty((5, nz, nx), device=dev, dtype=torch.float32)
        with torch.cuda.device(dev):
            _lib.check(lib.mifwi_elastic_materials(dev.index or 0, *[_lib.ptr(t) for t in ins], _lib.ptr(out), nz, nx,
                                                   float(s), int(bool(free_surface)), _stream()))
        ctx.save_for_backward(*ins)
        ctx.s, ctx.free_surface = float(s), int(bool(free_surface))
        return out

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        vp, vs, rho = ctx.saved_tensors
        dev = vp.device
        nz, nx = vp.shape
        g = g.to(dtype=torch.float32).contiguous()
        grads = [torch.empty_like(vp) for _ in range(3)]
        with torch.cuda.device(dev):
            _lib.check(lib.mifwi_elastic_materials_vjp(dev.index or 0, _lib.ptr(vp), _lib.ptr(vs), _lib.ptr(rho), _lib.ptr(g),
                                                       *[_lib.ptr(t) for t in grads], nz, nx, ctx.s, ctx.free_surface,
                                                       _stream()))
        return grads[0], grads[1], grads[2], None, None


PARAM_VELOCITY, PARAM_IMPEDANCE, PARAM_LAME = 1, 2, 3


def gradient_parametrization(prm, grads, mode):
    """Gradients with respect to (Vp, Vs, rho) -> the parameter set DENISE calls INVMAT1 (``models/networks.py:11025``):
    1 unchanged, 2 (Zp = rho Vp, Zs = rho Vs, rho), 3 (lambda, mu, rho).  ``prm`` = (vp, vs, rho), ``grads`` = the three
    gradients, float32 tensors of one shape on a HIP device; returns three new tensors.  One launch
    (``mifwi_elastic_gradient_parametrization``): the 3 x 3 Jacobian of the change of variables cell by cell.
    A term whose divisor is zero contributes 0, so the result is finite everywhere: where rho = 0 the first two
    gradients are 0 and the rho gradient passes unchanged; in the Lame form a cell with Vp = 0 has no lambda gradient
    and no Vp term in the mu gradient, and a cell with Vs = 0 no Vs term."""
    vp, vs, rho = (t.detach().contiguous().float() for t in prm)
    gv, gs, gr = (t.detach().contiguous().float() for t in grads)
    if not vp.is_cuda:
        raise MifwiError("gradient_parametrization: tensors must live on a HIP device (libmifwi has no CPU fallback)")
    out = [torch.empty_like(vp) for _ in range(3)]
    with torch.cuda.device(vp.device):
        _lib.check(_lib.load().mifwi_elastic_gradient_parametrization(
            vp.device.index or 0, int(mode), _lib.ptr(vp), _lib.ptr(vs), _lib.ptr(rho), _lib.ptr(gv), _lib.ptr(gs),
            _lib.ptr(gr), _lib.ptr(out[0]), _lib.ptr(out[1]), _lib.ptr(out[2]), vp.numel(), _stream()))
    return tuple(out)


def staggered_materials(vp, vs, rho, dt, h, free_surface=False):
    """[5, nz, nx] = lambda dt/h, (lambda+2mu) dt/h, mu_xz dt/h, dt/(h rho_x), dt/(h rho_z).
    With ``free_surface`` row 0 of the first two planes is put in the effective form the
    stress-imaging condition needs (szz = 0 there): lambda -> 0, lambda+2mu -> (lambda+2mu) -
    lambda^2/(lambda+2mu).

    Arithmetic averaging of density to the vx / vz nodes, harmonic averaging of the shear
    modulus to the sxz node (0 where any of the four is 0, i.e. in water), edge values
    replicated.  Differentiable.  Float32 tensors on a HIP device take the fused kernels of csrc/mifwi_materials.hip (the
    same operations in the same order: identical planes); anything else (CPU tensors of the tests' oracle compositions,
    float64) the plain torch expression below, which is the definition."""
    if (vp.is_cuda and vs.is_cuda and rho.is_cuda and vp.dim() == 2 and vp.shape == vs.shape == rho.shape and
            vp.dtype == vs.dtype == rho.dtype == torch.float32):
        return _MaterialsFn.apply(vp, vs, rho, dt / h, free_surface)
    return _staggered_materials_torch(vp, vs, rho, dt, h, free_surface)


def _staggered_materials_torch(vp, vs, rho, dt, h, free_surface=False):
    mu = rho * vs * vs
    lam = rho * vp * vp - 2.0 * mu
    s = dt / h

    def sh(a, dz, dx):
        a = torch.cat([a, a[-1:, :]], 0)[dz:dz + a.shape[0]] if dz else a
        a = torch.cat([a, a[:, -1:]], 1)[:, dx:dx + a.shape[1]] if dx else a
        return a
    rx = 0.5 * (rho + sh(rho, 0, 1))
    rz = 0.5 * (rho + sh(rho, 1, 0))
    m4 = [mu, sh(mu, 0, 1), sh(mu, 1, 0), sh(mu, 1, 1)]
    anyzero = (m4[0] == 0) | (m4[1] == 0) | (m4[2] == 0) | (m4[3] == 0)
    inv = sum(1.0 / torch.where(m == 0, torch.ones_like(m), m) for m in m4)
    muxz = torch.where(anyzero, torch.zeros_like(mu), 4.0 / inv)
    Ls, Ms = lam * s, (lam + 2.0 * mu) * s
    if free_surface:
        top = torch.zeros_like(Ls)
        top[0] = 1.0
        Ms = Ms - top * (Ls * Ls / Ms)
        Ls = Ls * (1.0 - top)
    return torch.stack([Ls, Ms, muxz * s, s / rx, s / rz])


class ElasticPlan(_Plan):
    PREFIX, LAYOUT = "elastic", _lib.ElasticLayout

    def __init__(self, nz, nx, nt, nshot, nsrc, nrec, ntap, pml_width, device_index,
                 shots_per_group=0, free_surface=0, source_type=0, record_pressure=0, snapshot_format=None,
                 fd_order=4):
        fmt = SNAPSHOT_FORMATS[snapshot_format or snapshot_mode()]
        self._create(_lib.ElasticDesc(nz, nx, nt, nshot, nsrc, nrec, ntap, pml_width,
                                      free_surface, shots_per_group, source_type, record_pressure, fmt, fd_order),
                     device_index)


class PseudoHessian(_MomentsHolder):
    """Holder of the six snapshot second moments behind the diagonal pseudo-Hessian (Shin's preconditioner; DENISE's
    ``EPRECOND = 1``): pass it to :func:`propagate` (``pseudo_hessian=``) and every backward pass through that call
    adds ``M0..M4 = sum Sk^2, M5 = sum S0 S1`` of its forward snapshot planes - summed over its shots and over the
    steps n with ``n % stride == 0``, each weighted by ``stride`` - into ``.moments`` [6, nz, nx] (None before the
    first backward).  The holder accumulates over calls (shot chunks, ranks' shares); :meth:`reset` zeroes it.
    The pass is one more read of the snapshot buffer the backward holds (``mifwi_elastic_snapshot_moments``), no
    extra propagation; ``stride = 4`` reads a quarter of it."""

    def hessian(self, vp, vs, rho, dt, h, parametrization=PARAM_VELOCITY):
        """[3, nz, nx]: the pseudo-Hessian planes of (Vp, Vs, rho), (Zp, Zs, rho) or (lambda, mu, rho) - the order of
        :func:`gradient_parametrization` - from the moments held and the model the run used:
        ``H_p = (L_p^2 + M_p^2)(M0 + M1) + 4 L_p M_p M5 + mu_p^2 M2 + b_p^2 (M3 + M4)`` with the parameter's pointwise
        partials of the collocated materials (include/mifwi.h has the table).  A collocated approximation: the
        staggered averages, the harmonic mu_xz and the effective row 0 under a free surface are ignored.  Finite and
        >= 0 everywhere (a term whose divisor is zero contributes 0)."""
        mom = self._held("hessian")
        _, nz, nx = mom.shape
        prm = self._model_planes("hessian", mom, (vp, vs, rho), (nz, nx))
        out = torch.empty((3, nz, nx), device=mom.device, dtype=torch.float32)
        with torch.cuda.device(mom.device):
            _lib.check(_lib.load().mifwi_elastic_pseudo_hessian(
                mom.device.index or 0, int(parametrization), _lib.ptr(prm[0]), _lib.ptr(prm[1]), _lib.ptr(prm[2]),
                _lib.ptr(mom), nz, nx, nx, float(dt) / float(h), _lib.ptr(out[0]), _lib.ptr(out[1]), _lib.ptr(out[2]),
                _stream()))
        return out


class _ArenaLease:
    """Held by the autograd node whose forward wrote the arena's tensor; dies with the node (a graph dropped without a
    backward frees the arena too)."""

    def __init__(self):
        self.released = False


class _SnapshotArena:
    """One snapshot tensor shared by consecutive propagate() calls (gradient_in_shot_chunks): the first call allocates
    it, later ones whose snapshots are not larger take a prefix - no call pays a malloc of >100 GB again, and chunks need
    not be of equal size to hit torch's cached block.  The tensor has ONE owner at a time: a forward leases it, the
    matching backward (or the death of its graph) gives it back; a second forward in between - two components, a
    forward inside a loss closure, retain_graph - does not get it and allocates snapshots of its own, so its
    predecessor's planes are never overwritten."""
    current = None

    def __init__(self):
        self.buf = None
        self._lease = None          # weakref to the _ArenaLease of the forward whose snapshots live in buf

    def __enter__(self):
        self._prev, _SnapshotArena.current = _SnapshotArena.current, self      # re-entering keeps the tensor
        return self

    def __exit__(self, *exc):
        _SnapshotArena.current = self._prev
        self.buf = None
        self._lease = None
        return False

    def busy(self):
        lease = self._lease() if self._lease is not None else None
        return lease is not None and not lease.released

    def lease(self):
        lease = _ArenaLease()
        self._lease = weakref.ref(lease)
        return lease

    def take(self, nt, elems, dev):
        need = nt * elems
        if self.busy() or self.buf is None or self.buf.device != dev or self.buf.numel() < need:
            return None
        return self.buf[:need].view(nt, elems)


class _Elastic(_psv.Psv, planes=5):
    """The isotropic scheme: what it has beyond :class:`_psv.Psv` - pressure receivers (bound to the plan), the snapshot
    arena and the plan's own say in the shot chunks.  opts: pml_width, shots_per_group, free_surface, source_type,
    record_pressure, snapshot_format, fd_order - the plan's."""
    name = "elastic"
    moment_planes = (6,)
    linearised_serves = ("%s serves explosive sources and velocity receivers only (force sources need df from the "
                         "density at the source node, pressure receivers a sampling pass of their own)")
    Plan = ElasticPlan
    traces = staticmethod(lambda o: 3 if o["record_pressure"] else 2)

    @classmethod
    def outputs(cls, plan, shape, dev, o):
        rec = super().outputs(plan, shape, dev, o)
        if o["record_pressure"]:      # pressure receivers: sum w (sxx + szz), bound to the plan
            _lib.check(_lib.load().mifwi_elastic_plan_bind_pressure(plan.handle, _lib.ptr(rec[2]), None))
        return rec

    @staticmethod
    def adjoint_sources(plan, g, shape, dev, o):
        g_p = None
        if o["record_pressure"]:
            g_p = None if g[2] is None or g[2].numel() == 0 else g[2].to(dtype=torch.float32).contiguous()
            # the forward re-runs of a checkpointed backward must not sample again: rec_p unbound
            _lib.check(_lib.load().mifwi_elastic_plan_bind_pressure(plan.handle, None, _lib.ptr(g_p)))
        # g_p is bound to the plan: the caller keeps it alive with the other two
        return _psv.Psv.adjoint_sources(plan, g, shape, dev, o) + [g_p]

    @staticmethod
    def snapshots(snapshot_budget, dev, nt, step):
        """The tensor of the current :class:`_SnapshotArena` when it is free and large enough (memory already held: no
        budget question); else as every propagator, and the first resident buffer inside an arena becomes the arena's."""
        arena = _SnapshotArena.current
        snap = arena.take(nt, step[0], dev) if arena is not None else None
        if snap is not None:
            return nt, snap, arena.lease()
        seg, snap, _ = Physics.snapshots(snapshot_budget, dev, nt, step)
        if snap is None or arena is None or arena.buf is not None:
            return seg, snap, None
        arena.buf = snap.view(-1)
        return seg, snap, arena.lease()

    @staticmethod
    def backward_done(lease):
        if lease is not None:               # the arena's tensor may serve the next forward
            lease.released = True

    @staticmethod
    def shot_chunk(make_plan, dims, budget):
        n0, n1, nt, ns = dims[:4]
        return resident_shot_chunk(ns, nt, n0, n1, budget, "f32")

    @staticmethod
    def chunk_plan(name, make_plan, c, nt, budget):
        for c in range(c, 0, -1):           # the plan's own plane size decides (column-blocked planes are padded)
            plan = make_plan(c)
            if 4 * nt * plan.layout.snap_step_elems <= budget:
                if plan.layout.snapshot_format != _lib.SNAPSHOT_F32:
                    plan.close()
                    raise MifwiError("%s reads f32 snapshot planes: this plan keeps them as bf16" % name)
                return plan
            plan.close()
        return None


def _options(pml_width, shots_per_group, free_surface, source_type, record_pressure, snapshot_format, fd_order):
    st = source_type_code(source_type)
    if snapshot_format is not None and snapshot_format not in SNAPSHOT_FORMATS:
        raise MifwiError("snapshot_format must be one of %s" % sorted(SNAPSHOT_FORMATS))
    return dict(pml_width=int(pml_width), shots_per_group=int(shots_per_group), free_surface=1 if free_surface else 0,
                source_type=st, record_pressure=1 if record_pressure else 0, snapshot_format=snapshot_format,
                fd_order=int(fd_order))


def propagate(mat, f, pz, px, src_cell, src_w, rec_cell, rec_w, pml_width,
              shots_per_group=0, snapshot_budget=DEFAULT_SNAPSHOT_BUDGET, free_surface=False,
              source_type="explosive", record_pressure=False, snapshot_format=None, fd_order=4, pseudo_hessian=None):
    """Elastic forward modelling, differentiable w.r.t. ``mat`` and ``f``.

    mat [5,nz,nx] from :func:`staggered_materials`;  f [nt,nshot,nsrc] (added to sxx and szz);
    source_type "explosive" (DENISE QUELLTYPB 1), or a point force "fx" / "fz" (QUELLTYPB 2 / 3): f is then
    added to vx / vz between the velocity and the stress update - scale it with
    :func:`force_amplitude` so that the density at the source node enters the gradient;
    pz [6,nz], px [6,nx] from :func:`profiles.cpml_tables`;  cells are iz*nx+ix.
    free_surface: row 0 is a stress-free surface (build ``mat`` with ``free_surface=True`` and
    ``pz`` with ``low=False``).
    fd_order: 4 (default) or 2 - spatial order of the staggered first derivatives (DENISE ``FD_ORDER``); the time
    step must respect the order's own stability limit (:func:`profiles.elastic_cfl_limit`).
    snapshot_format: "f32" (default; the gradient is the exact discrete adjoint) or "bf16": the forward snapshot
    planes are kept as bf16 (half the snapshot stream and memory; material gradients within 4e-3 rel-L2 of the
    f32 form in the worst case, seismograms unchanged) on grids that run the per-step kernels; None = MIFWI_EL_SNAP or "f32".
    pseudo_hessian: a :class:`PseudoHessian` holder, or None.  The backward pass through this call then adds the second
    moments of its snapshot planes into the holder (one more read of the snapshot buffer - resident, or every
    regenerated checkpoint segment once); a run that needs no gradient has no such pass and raises.  Without a holder
    nothing changes: the same launches, the same results.
    Cells may carry one tap of weight 1 or the four bilinear taps of a point ([nshot, npoint, 4], inactive taps -1;
    such runs use the one-launch-per-half-step kernels).  Repeated calls return the same seismograms bit for bit; the
    gradients are bit-repeatable while no cell receives more than two receiver taps of a shot.  With three or more
    (bilinear receivers closer than a cell) the per-step adjoint adds them with LDS float atomics in hardware order:
    the bits then differ from call to call (observed with four taps per cell), each call within 2e-5 rel-L2 of the
    fixed-order sum.
    Returns (rec_vx, rec_vz), each [nt,nshot,nrec], sampled after the velocity update; with
    ``record_pressure`` also rec_p = sum w (sxx + szz) at the receivers after the stress update (DENISE's
    pressure seismogram is ``-rec_p``; such runs use the one-launch-per-half-step kernels)."""
    _require_cuda(mat, "mat")
    geom = _Geometry.get(src_cell, src_w, rec_cell, rec_w, mat.device)
    f = f.to(device=mat.device)
    opts = _options(pml_width, shots_per_group, free_surface, source_type, record_pressure, snapshot_format, fd_order)
    if pseudo_hessian is not None and not isinstance(pseudo_hessian, PseudoHessian):
        raise MifwiError("pseudo_hessian must be an elastic.PseudoHessian holder or None")
    return Propagate.apply(mat, f, _Elastic, pz, px, geom, int(snapshot_budget), pseudo_hessian, opts)


def materials_jvp(vp, vs, rho, dvp, dvs, drho, dt, h, free_surface=False):
    """dmat [5, nz, nx]: the first-order change of :func:`staggered_materials` for the model perturbation
    (dvp, dvs, drho) - the forward-mode derivative of the torch expression that defines the planes, on the tensors'
    device and in their dtype; the transpose of the VJP autograd runs through ``staggered_materials``.  Finite where
    Vs = 0 (keep ``dvs`` = 0 there: water stays water); under ``free_surface`` row 0 of plane 0 is 0."""
    prm = [torch.as_tensor(t).detach() for t in (vp, vs, rho)]
    tan = [torch.as_tensor(t).detach().to(device=prm[0].device, dtype=prm[0].dtype) for t in (dvp, dvs, drho)]
    if any(t.shape != prm[0].shape for t in prm + tan) or prm[0].dim() != 2:
        raise MifwiError("materials_jvp: vp, vs, rho and their perturbations must be [nz, nx] tensors of one shape")
    return torch.func.jvp(lambda a, b, c: _staggered_materials_torch(a, b, c, dt, h, free_surface),
                          tuple(prm), tuple(tan))[1]


def _linearised(name, mat, dmat, f, pz, px, src_cell, src_w, rec_cell, rec_w, pml_width, df, free_surface, fd_order,
                snapshot_budget, source_type, record_pressure, snapshot_format, adjoint, weight):
    """born / gauss_newton_product through :func:`_driver.linearised`, over resident f32 snapshots.  Returns (background
    traces, perturbed traces, hv): lists of 2 tensors."""
    _require_cuda(mat, "mat")
    opts = _options(pml_width, 0, free_surface, source_type, record_pressure, snapshot_format, fd_order)
    return _psv.linearised(_Elastic, name, mat, dmat, f, df, pz, px, (src_cell, src_w, rec_cell, rec_w), snapshot_budget,
                           adjoint, weight, opts)


def born(mat, dmat, f, pz, px, src_cell, src_w, rec_cell, rec_w, pml_width, df=None, free_surface=False, fd_order=4,
         snapshot_budget=DEFAULT_SNAPSHOT_BUDGET, source_type="explosive", record_pressure=False, snapshot_format=None):
    """Born / linearised modelling: returns ``(rec_vx, rec_vz, drec_vx, drec_vz)`` - the seismograms of the background
    ``mat`` (what :func:`propagate` returns, bit for bit) and ``drec = J (dmat, df)``, their first-order change for the
    perturbation ``dmat`` [5, nz, nx] of the material planes (:func:`materials_jvp` maps (dVp, dVs, drho) to it) and,
    optionally, ``df`` [nt, nshot, nsrc] of the source amplitudes.  ``J`` is the exact transpose partner of the
    gradients autograd returns for :func:`propagate`.  No autograd through this call.

    One plan runs the background forward with resident f32 snapshots, in whichever kernel family it picks; the Born
    pass (``mifwi_elastic_born``, one launch per half step) then reads the same buffer.  When the snapshots of all shots
    do not fit ``snapshot_budget`` the shots are taken a few at a time (they are independent: the same results); when
    not even one shot fits, ``MifwiError`` - Born across time checkpoints is not served, nor are bf16 snapshot planes,
    force sources and pressure receivers (``source_type``, ``record_pressure``, ``snapshot_format`` are accepted so
    that a caller's propagate() arguments can be passed along, and refused)."""
    rec, drec, _ = _linearised("born", mat, dmat, f, pz, px, src_cell, src_w, rec_cell, rec_w, pml_width, df, free_surface,
                               fd_order, snapshot_budget, source_type, record_pressure, snapshot_format, False, None)
    return tuple(rec) + tuple(drec)


def gauss_newton_product(mat, dmat, f, pz, px, src_cell, src_w, rec_cell, rec_w, pml_width, df=None, free_surface=False,
                         fd_order=4, snapshot_budget=DEFAULT_SNAPSHOT_BUDGET, weight=None, source_type="explosive",
                         record_pressure=False, snapshot_format=None):
    """Gauss-Newton Hessian-vector product ``hv = J^T W J dmat`` [5, nz, nx] with ONE background forward, one Born pass
    and one adjoint pass over the same resident snapshot buffer (composing :func:`born` and :func:`propagate` runs the
    background twice).  Returns ``(hv, drec_vx, drec_vz)`` with ``drec = J (dmat, df)`` as :func:`born` gives it.

    ``weight``: None - the L2 misfit's identity - or a callable ``(drec_vx, drec_vz) -> (g_vx, g_vz)``: a data weighting,
    or the second derivative of another misfit.  Shots are taken a few at a time like :func:`born` when their
    snapshots do not fit the budget; ``hv`` sums over the chunks and ``weight`` is then called once per chunk with that
    chunk's [nt, shots, nrec] traces, so it must act shot by shot.  Other arguments and refusals as :func:`born`."""
    _, drec, hv = _linearised("gauss_newton_product", mat, dmat, f, pz, px, src_cell, src_w, rec_cell, rec_w, pml_width,
                              df, free_surface, fd_order, snapshot_budget, source_type, record_pressure, snapshot_format,
                              True, weight)
    return (hv,) + tuple(drec)


def resident_shot_chunk(nshot, nt, nz, nx, snapshot_budget=DEFAULT_SNAPSHOT_BUDGET, snapshot_format=None, device=None):
    """How many shots at a time keep the snapshots of ALL `nt` steps inside the budget (and inside 80 % of the memory
    that is free right now): ``nshot`` when everything fits, 0 when not even one shot does.

    :func:`propagate` cuts the time axis into checkpointed segments when the snapshots of a call do not fit, which
    costs one extra forward sweep.  When the misfit is known before the backward pass starts (observed data in hand,
    as in DENISE's ``grad`` or seisgan's ``FWILoss``) the cheaper cut is across SHOTS: they are independent, so a few at
    a time run forward with resident snapshots and straight into their adjoint, gradients adding up
    (:func:`gradient_in_shot_chunks`) - no recomputation at all."""
    per_shot = nt * nz * (4 * ((nx + 3) // 4)) * snapshot_bytes_per_cell(snapshot_format)
    budget = int(snapshot_budget)
    if device is not None and torch.cuda.is_available():
        budget = min(budget, int(0.8 * _lib.free_device_bytes(device)))
    return int(min(nshot, budget // max(per_shot, 1)))


snapshot_arena = _SnapshotArena          # `with elastic.snapshot_arena(): ...` around hand-written chunk loops


def gradient_in_shot_chunks(mat, f, pz, px, src_cell, src_w, rec_cell, rec_w, pml_width, loss_fn, chunk, **kw):
    """Loss and its gradient with the shots taken ``chunk`` at a time (see :func:`resident_shot_chunk`).

    ``loss_fn(rec_vx, rec_vz, shots)`` -> scalar loss of the shots in the slice ``shots`` (the total loss is their
    sum).  d loss / d mat is accumulated into ``mat.grad`` (``mat`` may be a non-leaf: the chain rule runs once, after
    the last chunk), d loss / d f into ``f.grad`` when ``f`` requires it.  Returns the detached total loss.  Other
    keyword arguments go to :func:`propagate`."""
    ns = f.shape[1]
    chunk = max(1, min(int(chunk), ns))
    leaf = mat.detach().requires_grad_(mat.requires_grad)
    total = None
    fgrad = torch.zeros_like(f) if f.requires_grad else None
    with _SnapshotArena():                   # the chunks share the snapshot tensor of the first (largest) one
        for a in range(0, ns, chunk):
            sl = slice(a, min(a + chunk, ns))
            fc = f[:, sl].detach().requires_grad_(f.requires_grad)
            out = propagate(leaf, fc, pz, px, src_cell[sl], src_w[sl], rec_cell[sl], rec_w[sl], pml_width, **kw)
            loss = loss_fn(out[0], out[1], sl)
            loss.backward()
            total = loss.detach() if total is None else total + loss.detach()
            if fgrad is not None:
                fgrad[:, sl] = fc.grad
    if mat.requires_grad:
        if mat.is_leaf:
            mat.grad = leaf.grad if mat.grad is None else mat.grad + leaf.grad
        else:
            mat.backward(leaf.grad)
    if fgrad is not None:
        if f.is_leaf:
            f.grad = fgrad if f.grad is None else f.grad + fgrad
        else:
            f.backward(fgrad)
    return total


def force_amplitude(wavelet, mat, src_cell, src_w, h, source_type):
    """Point-force amplitudes for :func:`propagate`: wavelet [nt,nshot,nsrc] (force per unit length, N/m)
    times dt/(h^2 rho) at the source node - DENISE's ``vx += DT * amp / (DH^2 rho)`` with
    mat[3] = dt/(h rho_x), mat[4] = dt/(h rho_z).  Differentiable w.r.t. ``mat``: the source term's share of
    the density gradient comes from autograd."""
    plane = mat[3 if SOURCE_TYPES[source_type] == 1 else 4].reshape(-1)
    cell = src_cell.to(device=mat.device, dtype=torch.long).clamp_min(0)
    w = src_w.to(device=mat.device, dtype=mat.dtype) * (src_cell.to(mat.device) >= 0)
    b = (plane[cell] * w).sum(dim=-1)                       # [nshot, nsrc]
    return wavelet.to(device=mat.device, dtype=mat.dtype) * (b / h)[None]
