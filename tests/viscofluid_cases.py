"""TEST INFRASTRUCTURE ONLY: what tests/test_viscofluid_host.py and tests/test_viscofluid_gpu.py share - the cases of
tests/test_fluid_gpu.py (its four shapes and its four-tap case, imported, not restated) with a seeded Q model, the cached
float64 references of tests/viscofluid_reference.py and the device helpers.

Q model: a smooth seeded qp = 20 + 180 u^3, f_relax 8 Hz, f_ref 30 Hz - the values of tests/psv_media.py and the reasons
given there.  "mat4": the four planes of viscofluid.materials (CPU float64, the definition, then rounded to f32, what the
device computes with); "matlim": the same model with qp = inf, the fluid's three planes and a zero plane.  Every reference
result is computed once per (case, source type, order) and left unchanged."""
import numpy as np
import torch

import viscofluid_reference as VR
from cases import FLUID_KINDS as KINDS, rel_l2
from psv_media import F_REF, F_RELAX, TOL_SUM, TOL_TRACE, f32, live_shots  # noqa: F401
from test_fluid_gpu import _CASES as FLUID_CASES, SHAPES  # noqa: F401

DEV = "cuda:0"
PLANES = ("K", "bx", "bz", "R")
ISO_OF = {"K": "K", "bx": "bx", "bz": "bz", "R": "K", "f": "f"}       # the lossless gradient whose error sets a plane's bound
_cache = {}


def q_model(nz, nx):
    rng = np.random.default_rng(31)
    z, x = np.meshgrid(np.arange(nz) / nz, np.arange(nx) / nx, indexing="ij")
    ph = 2 * np.pi * rng.random(2)
    u = 0.5 + 0.5 * np.sin(2 * np.pi * (1.3 * z + 0.7 * x) + ph[0]) * np.cos(2 * np.pi * 0.9 * x + ph[1])
    qp = 20 + 180 * u ** 3
    assert 20 <= qp.min() and qp.max() <= 200 and qp.std() > 10
    return f32(qp)


def case(key):
    """The fluid case ``key`` ((nz, nx, fs) or ("taps4", fs)) with its inputs rounded to f32, "qp", "mat4", "matlim",
    "relax" and seeded 1 % perturbations "dmat" of the planes and "df" of the source amplitudes.  Read-only."""
    if key not in _cache:
        from physicsbasedfwi2_amd import visco, viscofluid
        c = dict(FLUID_CASES[key]())
        nz, nx = c["vp"].shape
        c["qp"] = q_model(nz, nx)
        c["relax"] = visco.relaxation(F_RELAX, c["dt"])
        t = lambda a: torch.tensor(f32(a), dtype=torch.float64)
        mats = lambda qp: f32(viscofluid.materials(t(c["vp"]), t(c["rho"]), t(qp), F_REF, F_RELAX, c["dt"], c["h"],
                                                   free_surface=bool(c["fs"])).numpy())
        c["mat4"], c["matlim"] = mats(c["qp"]), mats(np.full((nz, nx), np.inf))
        assert all(np.abs(c["mat4"][k]).max() > 0 for k in range(4)) and not c["matlim"][3].any()
        for k in ("pz", "px", "f", "sw", "rw"):
            c[k] = f32(c[k])
        prng = np.random.default_rng(100)
        c["dmat"] = f32(0.01 * prng.standard_normal(c["mat4"].shape) * c["mat4"])
        c["df"] = f32(0.01 * prng.standard_normal(c["f"].shape) * np.abs(c["f"]).max())
        for v in c.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _cache[key] = c
    return _cache[key]


def geo(c):
    return c["sc"], c["sw"], c["rc"], c["rw"]


def g_of(*rec):
    """The adjoint sources of the gradient tests: seeded noise at the size of each trace set."""
    rng = np.random.default_rng(12)
    return [f32(rng.standard_normal(a.shape) * np.abs(a).max()) for a in rec]


def ref(key, st, order, which="mat4", grad=True):
    """The reference on ``which`` = "mat4" / "matlim": dict(rec [3, nt, ns, nrec], g, planes [4, nz, nx], f)."""
    k = ("ref", key, st, order, which)
    if k not in _cache or (grad and "planes" not in _cache[k]):
        c = case(key)
        kw = dict(free_surface=c["fs"], fd_order=order, source_type=st)
        if grad:
            rec, gm, gf, g = VR.gradients(c[which], c["pz"], c["px"], c["f"], *geo(c), g_of, c["relax"], **kw)
            out = dict(rec=np.stack(rec), g=g, planes=gm, f=gf)
        else:
            with torch.no_grad():
                out = dict(rec=np.stack([a.numpy() for a in VR.forward(c[which], c["pz"], c["px"], c["f"], *geo(c),
                                                                       c["relax"], **kw)]))
        for v in out.values():
            for a in (v if isinstance(v, list) else [v]):
                a.setflags(write=False)
        _cache[k] = out
    return _cache[k]


def ref_jvp(key, st, order):
    k = ("jvp", key, st, order)
    if k not in _cache:
        c = case(key)
        d = VR.jvp(c["mat4"], c["dmat"], c["pz"], c["px"], c["f"], c["df"], *geo(c), c["relax"], eps=1e-5,
                   free_surface=c["fs"], fd_order=order, source_type=st)
        d.setflags(write=False)
        _cache[k] = d
    return _cache[k]


def moved_from_the_limit(key, st, order):
    """rel-L2, shot by shot, between the reference's vx, vz traces in the medium and at qp = inf, over the live shots
    (psv_media's rule: some shot must move by more than a percent)."""
    a, b = ref(key, st, order, "mat4", grad=False)["rec"][:2], ref(key, st, order, "matlim", grad=False)["rec"][:2]
    return [rel_l2(a[:, :, s], b[:, :, s]) for s in live_shots(a, 1e-6)]


# ---- device helpers -----------------------------------------------------------------------------------------------------
def dev(a):
    a = np.asarray(a)
    return torch.tensor(a, device=DEV, dtype=torch.int32 if a.dtype.kind == "i" else torch.float32)


def args(c, mat, f=None):
    """(mat, f, pz, px, src_cell, src_w, rec_cell, rec_w, pml_width)"""
    return [mat, dev(c["f"]) if f is None else f] + [dev(c[k]) for k in ("pz", "px", "sc", "sw", "rc", "rw")] + [c["fw"]]


def run(c, mat_np, st, order, g=None, lossless=False, gs=0, **kw):
    """viscofluid.propagate (``lossless``: fluid.propagate on three planes) + backward with the adjoint sources ``g``:
    (traces [3] on the device, grad_mat, grad_f as float64)."""
    from physicsbasedfwi2_amd import fluid, viscofluid
    mat = dev(mat_np).requires_grad_(g is not None)
    f = dev(c["f"]).requires_grad_(g is not None)
    mod, more = (fluid, []) if lossless else (viscofluid, [F_RELAX, c["dt"]])
    out = mod.propagate(*args(c, mat, f), *more, free_surface=bool(c["fs"]), source_type=KINDS[st], record_pressure=True,
                        fd_order=order, shots_per_group=gs, **kw)
    if g is None:
        return [a.detach() for a in out]
    torch.autograd.backward(list(out), [dev(a) for a in g])
    return [a.detach() for a in out], mat.grad.double().cpu().numpy(), f.grad.double().cpu().numpy()


def host(tr):
    return torch.stack(list(tr)).double().cpu().numpy()
