"""Host code the acoustic and the elastic propagator share: the plan wrapper, the acquisition geometry and its cache,
the pseudo-Hessian holder's base, the padding of model inputs, and the snapshot budget, time-checkpoint schedule and the
two loops that walk it for the autograd functions.  torch is device memory and stream plumbing here; all arithmetic is
in libmifwi.so.
"""
import collections
import ctypes
import os

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
        import weakref
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
    """What the pseudo-Hessian holders of the two propagators share: the stride, the accumulated moments of one grid."""

    def __init__(self, stride=1):
        if int(stride) < 1:
            raise MifwiError("PseudoHessian: stride must be >= 1 (got %r)" % (stride,))
        self.stride = int(stride)
        self.moments = None

    def reset(self):
        if self.moments is not None:
            self.moments.zero_()

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
    receivers) into one buffer of ``[seg, *step_shape]``, which stands in the absolute step numbers of its segment."""
    regenerate = snap is None
    if regenerate:
        fwork = torch.empty(layout.work_forward_elems, device=ckpt[0].device, dtype=torch.float32)
        snap = torch.empty((seg,) + tuple(step_shape), device=fwork.device, dtype=torch.float32)
    for v in checkpoint_schedule(nt, seg, rule)[1]:
        if regenerate:
            if v.restore is not None:
                fwork[:layout.state_elems].copy_(ckpt[v.restore])
            forward(_lib.ptr(snap), _lib.ptr(fwork), v.b, v.e, ZERO_STATE if v.restore is None else 0)
        adjoint(_lib.ptr(snap), v.b, v.hi, v.lo, v.flags)
        if moments is not None:
            moments(_lib.ptr(snap), v.b, *v.moments)
