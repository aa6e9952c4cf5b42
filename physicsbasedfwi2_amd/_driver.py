"""Host code the three propagators (acoustic, elastic, fluid) share: the plan wrapper, the acquisition geometry and its
cache, the pseudo-Hessian holder's base, the padding of model inputs, the snapshot budget, the time-checkpoint schedule
and the two loops that walk it, and - around those loops - the one autograd function (:class:`Propagate`) and the one
Born / Gauss-Newton driver (:func:`linearised`).  What differs from physics to physics reaches them as a
:class:`Physics` description.  torch is device memory and stream plumbing here; all arithmetic is in libmifwi.so.
"""
import collections
import ctypes
import math
import os
import weakref

import torch

from . import _lib
from ._lib import FINALIZE, ZERO_STATE, MifwiError


class _Plan:
    """RAII wrapper of ``mifwi_<PREFIX>_plan`` (include/mifwi.h); a subclass names PREFIX and LAYOUT and builds the
    descriptor in its ``__init__``."""
    PREFIX = LAYOUT = None

    def _create(self, desc, device_index):
        self._lib = _lib.load()
        self.desc = desc
        self._h = ctypes.c_void_p()
        _lib.check(self._fn("create")(ctypes.byref(self._h), device_index, ctypes.byref(self.desc)))
        self.layout = self.LAYOUT()
        _lib.check(self._fn("layout")(self._h, ctypes.byref(self.layout)))

    def _fn(self, name):
        return getattr(self._lib, "mifwi_%s_plan_%s" % (self.PREFIX, name))

    @property
    def handle(self):
        return self._h

    def pass_sizes(self):
        """(forward, adjoint) units per pass of the per-step kernels over the time range: shots / shot groups
        (elastic), shot groups (acoustic) - what stays inside the Infinity Cache."""
        a, b = ctypes.c_int32(0), ctypes.c_int32(0)
        _lib.check(self._fn("pass_sizes")(self._h, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    def cluster_slabs(self, adjoint=False):
        """Row slabs per shot of the single-launch time loop (0: one launch per step / half step)."""
        return int(self._fn("cluster_slabs")(self._h, int(bool(adjoint))))

    def close(self):
        if self._h:
            self._fn("destroy")(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass


def _require_cuda(t, name):
    if not t.is_cuda:
        raise MifwiError("%s must live on a HIP device (got %s): libmifwi has no CPU fallback"
                         % (name, t.device))


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# Geometries already built from the caller's four tap tensors, when those live on the device (weak references + versions:
# an entry is used only while the very same, unmodified tensor objects are passed again).  A training loop passes the same
# acquisition every iteration: the validation of the cells (a host round trip that stalls the launch queue) is paid once.
# What the key can see: the tensor OBJECT, its version counter, its storage address and shape.  What it cannot see: a
# write that bypasses autograd's version counter (`t.data[...] = `, a kernel of another library writing through the raw
# pointer) - a caller that edits an acquisition in place that way must pass a new tensor, or set MIFWI_NO_GEOM_CACHE=1
# (every call then rebuilds and re-validates its geometry).  Negative cells are inactive taps by convention (the
# kernels skip them), so the validation bounds the cells from above only.
_GEOMETRIES = []


def _geom_key(t):
    return (t._version, t.data_ptr(), tuple(t.shape))


class _Geometry:
    """Device-resident sparse-point description shared by forward and backward."""

    @classmethod
    def get(cls, src_cell, src_w, rec_cell, rec_w, device):
        given = (src_cell, src_w, rec_cell, rec_w)
        # host tensors may alias numpy buffers (no version counter there): rebuilt every call
        if not all(t.is_cuda for t in given) or os.environ.get("MIFWI_NO_GEOM_CACHE", "0") not in ("", "0"):
            return cls(src_cell, src_w, rec_cell, rec_w, device)
        for refs, versions, dev, geom in _GEOMETRIES:
            if dev == device and all(r() is t for r, t in zip(refs, given)) and versions == tuple(_geom_key(t) for t in given):
                return geom
        geom = cls(src_cell, src_w, rec_cell, rec_w, device)
        _GEOMETRIES[:] = [e for e in _GEOMETRIES if all(r() is not None for r in e[0])][-15:]
        _GEOMETRIES.append((tuple(weakref.ref(t) for t in given), tuple(_geom_key(t) for t in given), device, geom))
        return geom

    def check_cells(self, ncell, what):
        """Every tap inside the grid (an out-of-grid cell would fault the kernels).  One host round trip, once per
        geometry."""
        if self._top is None:
            tops = [c.max() for c in (self.src_cell, self.rec_cell) if c.numel()]
            self._top = int(torch.stack(tops).max()) if tops else -1
        if self._top >= ncell:
            raise MifwiError("src_cell/rec_cell hold a cell outside the %s grid" % what)

    def __init__(self, src_cell, src_w, rec_cell, rec_w, device):
        self._top = None
        self.src_cell = src_cell.to(device=device, dtype=torch.int32).contiguous()
        self.src_w = src_w.to(device=device, dtype=torch.float32).contiguous()
        self.rec_cell = rec_cell.to(device=device, dtype=torch.int32).contiguous()
        self.rec_w = rec_w.to(device=device, dtype=torch.float32).contiguous()
        if self.src_cell.dim() != 3 or self.rec_cell.dim() != 3:
            raise MifwiError("src_cell/rec_cell must be [nshot, npoint, ntap]")
        if self.src_cell.shape != self.src_w.shape or self.rec_cell.shape != self.rec_w.shape:
            raise MifwiError("cell/weight shape mismatch")
        if self.src_cell.shape[0] != self.rec_cell.shape[0]:
            raise MifwiError("source and receiver shot counts differ")
        if self.src_cell.shape[2] != self.rec_cell.shape[2]:
            raise MifwiError("sources and receivers must use the same number of taps")


class _MomentsHolder:
    """What the pseudo-Hessian holders of the three propagators share: the stride, the accumulated moments of one grid,
    and what their ``hessian*`` methods do before their own C call."""

    def __init__(self, stride=1):
        if int(stride) < 1:
            raise MifwiError("PseudoHessian: stride must be >= 1 (got %r)" % (stride,))
        self.stride = int(stride)
        self.moments = None

    def reset(self):
        if self.moments is not None:
            self.moments.zero_()

    def _held(self, what):
        """The moments, contiguous; refuses a holder no backward pass has filled."""
        if self.moments is None:
            raise MifwiError("PseudoHessian.%s: no moments yet - run a backward pass through "
                             "propagate(..., pseudo_hessian=holder) first" % what)
        return self.moments.contiguous()

    @staticmethod
    def _model_planes(what, mom, planes, shape, detail="like the moments", valid=True):
        """The model ``planes`` as contiguous float32 tensors on the moments' device; refuses when one is not of ``shape``
        (or the caller found its arguments not ``valid``), ``detail`` - which may name %(got)s - ending the message."""
        prm = [torch.as_tensor(t).detach().to(device=mom.device, dtype=torch.float32).contiguous() for t in planes]
        if not valid or any(tuple(t.shape) != tuple(shape) for t in prm):
            raise MifwiError("PseudoHessian.%s: the model must be [%d, %d] %s"
                             % (what, shape[0], shape[1], detail % {"got": tuple(prm[0].shape)}))
        return prm

    def _add(self, m):
        if self.moments is None:
            self.moments = m.contiguous().clone()
        elif self.moments.shape != m.shape or self.moments.device != m.device:
            raise MifwiError("PseudoHessian holds moments of a %s grid, this run has %s"
                             % (tuple(self.moments.shape[-2:]), tuple(m.shape[-2:])))
        else:
            self.moments.add_(m)


def ptrs(*tensors):
    return tuple(_lib.ptr(t) for t in tensors)


def pad_columns(t, gp, fill=0.0):
    """``t`` [..., n] -> float32 [..., gp] on the same device, the pad columns ``fill`` (the row layout of the model
    inputs in include/mifwi.h)."""
    shape = tuple(t.shape[:-1]) + (gp,)
    out = (torch.full(shape, fill, device=t.device, dtype=torch.float32) if fill else
           torch.zeros(shape, device=t.device, dtype=torch.float32))
    out[..., :t.shape[-1]] = t.detach()
    return out


def segment_length(snapshot_budget, dev, step_bytes, nt):
    """Steps per time-checkpoint segment; ``nt``: the snapshots of the whole run stay resident.  A segment holds its
    snapshots and leaves as much again to the checkpoints.  Never plans for more than most of the memory that is free
    right now (other tensors of the training loop share the device); segmentation does not change the results."""
    budget = min(snapshot_budget, int(0.8 * _lib.free_device_bytes(dev)))
    if nt * step_bytes <= budget:
        return nt
    return min(nt, max(1, int(budget // (2 * step_bytes))))


# Adjoint step k reads the snapshot of forward step k - lag.  Acoustic: G^{k-1} is the virtual source of step k, k = nt-1
# .. 1 (G^{nt-1} never reaches a recorded sample); elastic: the planes of step n serve adjoint step n, n = nt-1 .. 0.
SNAPSHOT_LAG = {"acoustic": 1, "elastic": 0}

# One backward visit: re-run forward steps [b, e) from checkpoint `restore` (None: from the zero state) into the segment's
# snapshot buffer, run adjoint steps hi .. lo with `flags`, hand the snapshot steps `moments` = [first, end) to the
# pseudo-Hessian pass.
Visit = collections.namedtuple("Visit", "b e restore hi lo flags moments")


def _segments(nt, seg):
    return [(b, min(b + seg, nt), ZERO_STATE if b == 0 else 0) for b in range(0, nt, seg)]


def checkpoint_schedule(nt, seg, rule):
    """The time-checkpoint schedule of ``nt`` steps in segments of ``seg`` (``seg >= nt``: one segment, the resident
    form), integers only.  Returns ``(segments, visits)``: the forward segments ``(b, e, flags)`` in order - the state is
    checkpointed at every b > 0, checkpoint i at the start of segment i + 1 - and the backward visits in issue order,
    last segment first.  A segment whose snapshots serve no adjoint step (the acoustic one-step segment at nt - 1) has
    no visit.  ZERO_STATE goes to the first segment and the first adjoint range issued, FINALIZE to the range of the
    segment that starts at 0, the last one issued."""
    lag = SNAPSHOT_LAG[rule]
    segments = _segments(nt, seg)
    visits = []
    for si in reversed(range(len(segments))):
        b, e, _ = segments[si]
        hi, lo = min(e - 1 + lag, nt - 1), b + lag
        if hi < lo:
            continue
        flags = (0 if visits else ZERO_STATE) | (FINALIZE if b == 0 else 0)
        visits.append(Visit(b, e, si - 1 if b else None, hi, lo, flags, (lo - lag, hi - lag + 1)))
    return segments, visits


def run_forward(forward, nt, seg, work, state_elems, snap=None):
    """The forward pass of an autograd function: ``forward(snap_ptr, work_ptr, b, e, flags)`` over the segments of
    ``seg`` steps.  ``seg == nt``: one call that writes its snapshots into ``snap`` (None: a run that needs no
    gradient).  Otherwise no snapshots yet: returns the state (the time levels and the C-PML memory variables, the first
    ``state_elems`` of ``work``) as it stood at every segment start after 0."""
    ckpt = []
    for b, e, flags in _segments(nt, seg):
        if b > 0:
            ckpt.append(work[:state_elems].clone())
        forward(_lib.ptr(snap), _lib.ptr(work), b, e, flags)
    return ckpt


def run_backward(rule, nt, seg, snap, adjoint, moments=None, forward=None, ckpt=None, layout=None, step_shape=None):
    """The adjoint pass over the visits of the schedule: ``adjoint(snap_ptr, snap_first, hi, lo, flags)``, then
    ``moments(snap_ptr, snap_first, first, end)`` when a pseudo-Hessian holder asks for it.  ``snap``: the resident
    snapshots of the forward pass (``seg == nt``), or None - each visit then restores its checkpoint from ``ckpt``
    (what :func:`run_forward` returned) and re-runs ``forward`` (as :func:`run_forward` takes it, sampling no
    receivers) into one buffer of ``[seg, *step_shape]``, which stands in the absolute step numbers of its segment.
    Returns the number of visits: 0 when the run has no adjoint step at all."""
    regenerate = snap is None
    if regenerate:
        fwork = torch.empty(layout.work_forward_elems, device=ckpt[0].device, dtype=torch.float32)
        snap = torch.empty((seg,) + tuple(step_shape), device=fwork.device, dtype=torch.float32)
    visits = checkpoint_schedule(nt, seg, rule)[1]
    for v in visits:
        if regenerate:
            if v.restore is not None:
                fwork[:layout.state_elems].copy_(ckpt[v.restore])
            forward(_lib.ptr(snap), _lib.ptr(fwork), v.b, v.e, ZERO_STATE if v.restore is None else 0)
        adjoint(_lib.ptr(snap), v.b, v.hi, v.lo, v.flags)
        if moments is not None:
            moments(_lib.ptr(snap), v.b, *v.moments)
    return len(visits)


class Physics:
    """What :class:`Propagate` and :func:`linearised` need to know of one propagator: a namespace of data attributes and
    static functions (never instantiated), one subclass per physics module.  ``opts`` is the module's own dict of plan
    options, passed through untouched; ``dims`` is (n0, n1, nt, nshot, nsrc, nrec, ntap).

    A subclass gives ``inputs(model, t0, t1, gp, opts)`` (the three coefficient tensors as the C calls take them),
    ``traces(opts)`` (how many receiver tensors a run has), ``forward_call(plan, coef, f_d, geo, rec)`` (``rec`` None: a
    re-run that samples nothing), ``adjoint_call(plan, coef, geo, g, grad, grad_f, work)`` and
    ``born_call(plan, coef, dmodel_p, df_d, geo, snap, drec, work, nt)``, and replaces what differs of the rest:
    ``plan`` (opts are the plan's keywords), ``snap_step`` (the shape of one step's snapshots), ``outputs`` (the receiver
    tensors of a forward), ``adjoint_sources`` (what the adjoint call gets of autograd's ``g``; None: no source)."""
    name = None                 # in messages and in the names of the C entry points
    rule = None                 # SNAPSHOT_LAG key: which snapshots an adjoint step reads
    model = None                # the model argument's name in messages
    grad_planes = ()            # leading dimensions of the model gradient and of the moments, in front of [n0, gp]
    moment_planes = ()
    zero_moments = False        # True: the moments start from 0 and every range adds; else the range that ends the run,
    #                             the first one issued, overwrites them
    not_served = None           # how the refusal of a budget below one shot ends
    weight_returns = None       # what follows "weight must return "; may name %(n)d, the number of traces
    Plan = None                 # the _Plan subclass

    @classmethod
    def plan(cls, dims, device_index, opts):
        return cls.Plan(*dims, device_index=device_index, **opts)

    @staticmethod
    def snap_step(lay, ns):
        return (lay.snap_step_elems,)

    @classmethod
    def outputs(cls, plan, shape, dev, opts):
        return _empty(cls.traces(opts), shape, dev)

    @staticmethod
    def adjoint_sources(plan, g, shape, dev, opts):
        return [None if t is None or t.numel() == 0 else t.to(dtype=torch.float32).contiguous() for t in g]

    @staticmethod
    def snapshots(snapshot_budget, dev, nt, step):
        """Where the snapshots of a forward that needs a gradient go: ``(seg, snap, lease)`` - the segment length, the
        resident buffer (None when seg < nt: time checkpoints) and whatever ``backward_done`` wants back."""
        seg = segment_length(snapshot_budget, dev, 4 * math.prod(step), nt)
        return seg, (torch.empty((nt,) + tuple(step), device=dev, dtype=torch.float32) if seg == nt else None), None

    @staticmethod
    def backward_done(lease):
        """The backward pass has read the snapshots for the last time."""

    @classmethod
    def shot_chunk(cls, make_plan, dims, budget):
        """Shots per chunk of a linearised pass: a one-shot plan tells the bytes of a shot's snapshots."""
        one = make_plan(1)
        chunk = min(dims[3], budget // (4 * dims[2] * math.prod(cls.snap_step(one.layout, 1))))
        one.close()
        return chunk

    @staticmethod
    def chunk_plan(name, make_plan, c, nt, budget):
        """The plan of the next chunk, of at most ``c`` shots; None: not even one shot fits."""
        return make_plan(c)

    @staticmethod
    def weigh(weight, drec):
        """The caller's ``weight`` on a chunk's perturbed traces, as a sequence of adjoint sources."""
        return weight(*drec)


def _dims(model, f, geom):
    """(n0, n1, nt, nshot, nsrc, nrec, ntap) of a run, checked against the geometry."""
    n0, n1 = model.shape[-2:]
    nt, ns, nsrc = f.shape
    if geom.src_cell.shape[:2] != (ns, nsrc):
        raise MifwiError("f is [nt,%d,%d] but src_cell is %s" % (ns, nsrc, tuple(geom.src_cell.shape)))
    geom.check_cells(n0 * n1, "%dx%d" % (n0, n1))
    return n0, n1, nt, ns, nsrc, geom.rec_cell.shape[1], geom.rec_cell.shape[2]


def _empty(n, shape, dev):
    return [torch.empty(shape, device=dev, dtype=torch.float32) for _ in range(n)]


class Propagate(torch.autograd.Function):
    """The autograd function of every propagator: ``apply(model, f, phys, t0, t1, geom, snapshot_budget, pseudo_hessian,
    opts)`` -> the tuple of receiver tensors ``phys.outputs`` allocates; differentiable w.r.t. ``model`` and ``f``."""

    @staticmethod
    def forward(ctx, model, f, phys, t0, t1, geom, snapshot_budget, hess, opts):
        _require_cuda(model, phys.model)
        dev = model.device
        dims = _dims(model, f, geom)
        nt, ns, nrec = dims[2], dims[3], dims[5]
        with torch.cuda.device(dev):
            plan = phys.plan(dims, dev.index, opts)
            lay = plan.layout
            coef = phys.inputs(model, t0, t1, lay.gp, opts)
            f_d = f.detach().to(dtype=torch.float32).contiguous()
            rec = phys.outputs(plan, (nt, ns, nrec), dev, opts)
            work = torch.empty(lay.work_forward_elems, device=dev, dtype=torch.float32)
            need_grad = model.requires_grad or f.requires_grad
            if hess is not None and not need_grad:
                raise MifwiError("pseudo_hessian: the moments are taken from the snapshots of a backward pass, and "
                                 "neither %s nor f requires a gradient in this run" % phys.model)
            seg, snap, lease = nt, None, None
            if need_grad:
                seg, snap, lease = phys.snapshots(snapshot_budget, dev, nt, phys.snap_step(lay, ns))
            geo = ptrs(geom.src_cell, geom.src_w, geom.rec_cell, geom.rec_w)
            ckpt = run_forward(phys.forward_call(plan, ptrs(*coef), f_d, geo, rec), nt, seg, work, lay.state_elems, snap)
            if need_grad:
                ctx.phys, ctx.opts, ctx.plan, ctx.geom, ctx.dims = phys, opts, plan, geom, dims
                ctx.seg, ctx.ckpt, ctx.snap, ctx.lease = seg, ckpt, snap, lease
                ctx.need_f = f.requires_grad
                ctx.hess = hess
                ctx.save_for_backward(*coef, f_d)
            else:
                plan.close()
        return tuple(rec)

    @staticmethod
    def backward(ctx, *g):
        lib = _lib.load()
        phys = ctx.phys
        if ctx.plan is None:
            raise MifwiError("backward through the %s propagator was called twice: the forward snapshots "
                             "(or checkpoints) are freed by the first call - run the forward again" % phys.name)
        *coef_t, f_d = ctx.saved_tensors
        plan, geom = ctx.plan, ctx.geom
        lay = plan.layout
        n0, n1, nt, ns, nsrc, nrec, _ = ctx.dims
        dev = f_d.device
        with torch.cuda.device(dev):
            g = phys.adjoint_sources(plan, g, (nt, ns, nrec), dev, ctx.opts)
            grad = torch.empty(phys.grad_planes + (n0, lay.gp), device=dev, dtype=torch.float32)
            grad_f = torch.zeros((nt, ns, nsrc), device=dev, dtype=torch.float32) if ctx.need_f else None
            work = torch.empty(lay.work_backward_elems, device=dev, dtype=torch.float32)
            hess = ctx.hess
            moments = None
            if hess is not None:
                mom = (torch.zeros if phys.zero_moments else torch.empty)(phys.moment_planes + (n0, lay.gp), device=dev,
                                                                          dtype=torch.float32)
                entry = "mifwi_%s_snapshot_moments" % phys.name
                mwork = torch.empty(getattr(lib, entry + "_work_elems")(plan.handle), device=dev, dtype=torch.float32)

                def moments(snap, first, b, e):
                    # one more read of a snapshot range this pass has in hand, each range once (absolute step numbers, so
                    # segments select the steps the resident buffer would)
                    _lib.check(getattr(lib, entry)(
                        plan.handle, snap, first, b, e, hess.stride, _lib.ptr(mom), _lib.ptr(mwork),
                        ZERO_STATE if e == nt and not phys.zero_moments else 0, _stream()))
            coef = ptrs(*coef_t)
            geo = ptrs(geom.src_cell, geom.src_w, geom.rec_cell, geom.rec_w)
            if not run_backward(phys.rule, nt, ctx.seg, ctx.snap, phys.adjoint_call(plan, coef, geo, g, grad, grad_f, work),
                                moments, phys.forward_call(plan, coef, f_d, geo, None), ctx.ckpt, lay, phys.snap_step(lay, ns)):
                grad.zero_()                     # no visit (acoustic, nt < 2: no adjoint step): nothing wrote the gradient
            if hess is not None:
                hess._add(mom[..., :n1])
                ctx.hess = None
            plan.close()
            ctx.plan = ctx.snap = ctx.ckpt = None
            phys.backward_done(ctx.lease)
            ctx.lease = None
        return (grad[..., :n1].contiguous(), grad_f) + (None,) * 7


def linearised(phys, name, model, dmodel, f, df, t0, t1, taps, snapshot_budget, adjoint, weight, opts):
    """born / gauss_newton_product of every propagator: per shot chunk one plan, one background forward with resident
    snapshots, the Born pass over that buffer and - ``adjoint`` - the adjoint pass over it too, ``weight`` (None: the
    identity) between the two.  The module has validated its own arguments.  Returns ``(rec, drec, hv)``: the background
    and the perturbed traces, lists of ``phys.traces(opts)`` tensors, and the product; rec is None with ``adjoint``, hv
    without.  No autograd through this call."""
    dev = model.device
    geom = _Geometry.get(*taps, dev)
    dims = _dims(model, f, geom)
    n0, n1, nt, ns, nsrc, nrec, ntap = dims
    if df is not None and tuple(df.shape) != tuple(f.shape):
        raise MifwiError("df must have the shape of f, %s (got %s)" % (tuple(f.shape), tuple(df.shape)))
    ntr = phys.traces(opts)

    def make_plan(c):
        return phys.plan((n0, n1, nt, c, nsrc, nrec, ntap), dev.index, opts)
    with torch.cuda.device(dev), torch.no_grad():
        f_d = f.detach().to(device=dev, dtype=torch.float32).contiguous()
        df_d = None if df is None else df.detach().to(device=dev, dtype=torch.float32).contiguous()
        rec = None if adjoint else _empty(ntr, (nt, ns, nrec), dev)
        drec = _empty(ntr, (nt, ns, nrec), dev)
        hv = torch.zeros(phys.grad_planes + (n0, n1), device=dev, dtype=torch.float32) if adjoint else None
        budget = min(int(snapshot_budget), int(0.8 * _lib.free_device_bytes(dev)))
        chunk = phys.shot_chunk(make_plan, dims, budget)
        a = 0
        while a < ns:
            plan = phys.chunk_plan(name, make_plan, min(chunk, ns - a), nt, budget) if chunk >= 1 else None
            if plan is None:
                raise MifwiError("%s keeps the forward snapshots of all %d steps resident, and not even one shot's fit the "
                                 "snapshot budget; %s" % (name, nt, phys.not_served))
            try:
                lay = plan.layout
                c = plan.desc.nshot
                sl = slice(a, a + c)
                coef_t = phys.inputs(model, t0, t1, lay.gp, opts)
                dmodel_p = pad_columns(dmodel.to(dev), lay.gp)
                taps_c = [t[sl].contiguous() for t in (geom.src_cell, geom.src_w, geom.rec_cell, geom.rec_w)]
                coef, geo = ptrs(*coef_t), ptrs(*taps_c)
                fc = f_d[:, sl].contiguous()
                dfc = None if df_d is None else df_d[:, sl].contiguous()
                # Born modelling of all shots at once writes its outputs in place; a product's traces stay the chunk's own
                # tensors, which is what the caller's weight() gets
                in_place = c == ns and not adjoint
                rec_c, drc = (rec, drec) if in_place else (_empty(ntr, (nt, c, nrec), dev) for _ in range(2))
                work = torch.empty(max(lay.work_forward_elems, lay.work_backward_elems if adjoint else 0), device=dev,
                                   dtype=torch.float32)
                snap = torch.empty((nt,) + tuple(phys.snap_step(lay, c)), device=dev, dtype=torch.float32)
                run_forward(phys.forward_call(plan, coef, fc, geo, rec_c), nt, nt, work, lay.state_elems, snap)
                phys.born_call(plan, coef, dmodel_p, dfc, geo, snap, drc, work, nt)
                if not in_place:
                    for k in range(ntr):
                        drec[k][:, sl] = drc[k]
                        if rec is not None:
                            rec[k][:, sl] = rec_c[k]
                if adjoint and checkpoint_schedule(nt, nt, phys.rule)[1]:       # a run without a visit has no adjoint step
                    g = drc if weight is None else phys.weigh(weight, drc)
                    g = [t.detach().to(device=dev, dtype=torch.float32).contiguous() for t in g]
                    if len(g) != ntr or any(t.shape != drc[0].shape for t in g):
                        raise MifwiError("weight must return " + phys.weight_returns % {"n": ntr})
                    grad = torch.empty(phys.grad_planes + (n0, lay.gp), device=dev, dtype=torch.float32)
                    run_backward(phys.rule, nt, nt, snap, phys.adjoint_call(plan, coef, geo, g, grad, None, work))
                    hv += grad[..., :n1]
            finally:
                plan.close()
            a += c
    return rec, drec, hv
