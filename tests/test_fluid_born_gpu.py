"""Fluid Born modelling (fluid.born / mifwi_fluid_born), the Gauss-Newton product (fluid.gauss_newton_product) and
fluid.materials_jvp.

Reference for J: the central difference (F(mat5 + eps d5) - F(mat5 - eps d5)) / 2 eps of the fp64 oracle's elastic forward
with pressure receivers, eps = 1e-5, on mat5 = [K, K, 0, bx, bz] and d5 = [dK, dK, 0, dbx, dbz], inputs rounded to f32
first.  Bound 2e-6 rel-L2 over (dvx, dvz) together and over drec_p: the project's bound for elastic.born against the same
reference (tests/test_elastic_born_gpu.py; the recursion is the same arithmetic).
Largest values measured on the MI355X over the 48 cases: 1.70e-6 (dvx, dvz) and 9.62e-7 (drec_p), both under a free surface;
the docstring of test_born_is_the_directional_derivative_of_the_oracle has the cases.
Dot-product and Gauss-Newton identities: 2e-5, the project's bound for sums taken in another order.
Shapes: those of tests/test_fluid_gpu.py (every tile form), 3 shots, 13 receivers on rows 15 | 16, nt = 60."""
import functools

import numpy as np
import pytest
import torch

from cases import FLUID_KINDS as KINDS, elastic_case, fluid_backward, fluid_planes, fluid_run, rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(37, 70), (37, 133), (44, 120), (23, 240)]
EPS = 1e-5
NT = 60


def _f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def _case(nz, nx, fs, seed=0):
    """The case of tests/test_fluid_gpu.py at nt = 60 with its real inputs rounded to f32, a seeded 1 % perturbation of the
    three material planes (row 0 of dK zero under a free surface) and one of the source amplitudes."""
    c = elastic_case(seed=7, nz=nz, nx=nx, fw=6, nt=NT, ns=3, nsrc=1, nrec=13, water=0, free_surface=bool(fs))
    sc = c["sc"].copy()
    sc[0, 0, 0] = (sc[0, 0, 0] // nx) * nx + 3          # inside the C-PML on the left
    if fs:
        sc = np.where(sc // nx == 0, sc + nx, sc)       # off the surface row
        assert (sc // nx >= 1).all()
    c["sc"] = sc.astype(np.int32)
    rx = np.linspace(2, nx - 3, 13).astype(int)
    rows = [0 if fs else 15, 16, 15]
    c["rc"] = np.stack([(r * nx + rx) for r in rows])[:, :, None].astype(np.int32)
    c["rw"] = np.ones(c["rc"].shape)
    c = fluid_planes(c, fs)
    for k in ("pz", "px", "f", "sw", "rw"):
        c[k] = _f32(c[k])
    rng = np.random.default_rng(100 + seed)
    c["dmat"] = (0.01 * rng.standard_normal(c["mat3"].shape) * c["mat3"]).astype(np.float32)
    if fs:
        c["dmat"][0, 0] = 0.0
    c["df"] = (0.01 * rng.standard_normal(c["f"].shape) * np.abs(c["f"]).max()).astype(np.float32)
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def _oracle_jvp(nz, nx, fs, order, st):
    """Central difference of the fp64 oracle's forward, computed once per case and left unchanged: (dvx, dvz), drec_p."""
    import oracle
    o64 = oracle.load("f64")
    c = _case(nz, nx, fs)
    d = c["dmat"].astype(np.float64)
    d5 = np.stack([d[0], d[0], np.zeros_like(d[0]), d[1], d[2]])
    m5 = c["mat5"].astype(np.float64)
    run = lambda m: o64.elastic_forward(m, c["pz"], c["px"], c["f"], c["sc"], c["sw"], c["rc"], c["rw"],
                                        free_surface=c["fs"], source_type=st, pressure=True, fd_order=order)
    p, m = run(m5 + EPS * d5), run(m5 - EPS * d5)
    dv = np.stack([(p[0] - m[0]) / (2 * EPS), (p[1] - m[1]) / (2 * EPS)])
    dp = (p[2] - m[2]) / (2 * EPS)
    dv.setflags(write=False)
    dp.setflags(write=False)
    return dv, dp


def _t(a):
    a = np.asarray(a)
    return torch.tensor(a, device=DEV, dtype=torch.int32 if a.dtype.kind == "i" else torch.float32)


def _args(c):
    """(f, pz, px, src_cell, src_w, rec_cell, rec_w, pml_width) of born() behind mat and dmat."""
    return [_t(c[k]) for k in ("f", "pz", "px", "sc", "sw", "rc", "rw")] + [c["fw"]]


def _born(c, st=0, order=4, dmat=None, df=None, pressure=True, **kw):
    from physicsbasedfwi2_amd import fluid
    dm = _t(c["dmat"]) if dmat is None else dmat
    return fluid.born(_t(c["mat3"]), dm, *_args(c), df=df, free_surface=bool(c["fs"]), source_type=KINDS[st],
                      record_pressure=pressure, fd_order=order, **kw)


def _gn(c, dmat, st=0, **kw):
    from physicsbasedfwi2_amd import fluid
    return fluid.gauss_newton_product(_t(c["mat3"]), dmat, *_args(c), free_surface=bool(c["fs"]), source_type=KINDS[st],
                                      record_pressure=True, **kw)


def _dot(a, b):
    return float((a.double() * b.double()).sum())


def _dots(xs, ys):
    return sum(_dot(a, b) for a, b in zip(xs, ys))


def _stack(ts):
    return torch.stack(list(ts)).double().cpu().numpy()


def _close(a, b, tol, what):
    print("%s: %.9e vs %.9e, |diff| / max = %.2e" % (what, a, b, abs(a - b) / max(abs(a), abs(b))))
    assert abs(a - b) <= tol * max(abs(a), abs(b)), what


def _adjoint_source(drec):
    return [torch.sign(a) + 0.5 for a in drec]


def _gradient(c, st, g, order=4):
    """fluid.propagate + backward with the adjoint sources g (vx, vz, p): the leaves (mat, f)."""
    mat, f, out = fluid_run(c, st, order)
    fluid_backward(out, [a.cpu().numpy() for a in g])
    return mat, f


# ---- 1: directional derivative against the fp64 oracle ------------------------------------------------------------
@pytest.mark.parametrize("st", [0, 1, 2], ids=["explosive", "fx", "fz"])
@pytest.mark.parametrize("order", [2, 4])
@pytest.mark.parametrize("fs", [0, 1], ids=["absorbing_top", "free_surface"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_born_is_the_directional_derivative_of_the_oracle(shape, fs, order, st):
    """Largest values measured on the MI355X over the 48 cases: 1.70e-6 over (dvx, dvz) (23x240, free surface, order 2,
    explosive; 4.7e-8 to 1.7e-6 over the cases) and 9.62e-7 over drec_p (37x70, free surface, order 2, explosive; 3.7e-8
    to 9.6e-7).  The six values above 7.8e-7 are all free-surface cases, whose shot 0 is recorded on the surface row."""
    nz, nx = shape
    c = _case(nz, nx, fs)
    want_v, want_p = _oracle_jvp(nz, nx, fs, order, st)
    out = _born(c, st, order)
    assert len(out) == 6
    got_v, got_p = _stack(out[3:5]), out[5].double().cpu().numpy()
    ev, ep = rel_l2(got_v, want_v), rel_l2(got_p, want_p)
    print("born vs fp64 central difference, %dx%d fs=%d order=%d st=%d: rel-L2 v %.3e p %.3e" % (nz, nx, fs, order, st, ev, ep))
    assert np.abs(want_v).max() > 0 and np.abs(want_p).max() > 0
    assert np.abs(got_v).max() > 0 and np.abs(got_p).max() > 0
    assert ev <= 2e-6
    assert ep <= 2e-6


# ---- 2: the background traces are untouched -----------------------------------------------------------------------
@pytest.mark.parametrize("pressure", [True, False], ids=["with_p", "without_p"])
def test_background_traces_equal_propagate(pressure):
    c = _case(37, 133, 1)
    out = _born(c, 1, pressure=pressure)
    n = 3 if pressure else 2
    assert len(out) == 2 * n
    _, _, ref = fluid_run(c, 1, 4, record_pressure=pressure, mat_grad=False, f_grad=False)
    assert len(ref) == n
    for a, b in zip(out[:n], ref):
        assert a.abs().max() > 0 and torch.equal(a, b)
    full = _born(c, 1)
    for a, b in zip(out[n:], full[3:3 + n]):           # the perturbed velocity traces do not depend on the pressure output
        assert torch.equal(a, b)


# ---- 3: transpose partner of the gradients ------------------------------------------------------------------------
@pytest.mark.parametrize("fs", [0, 1], ids=["absorbing_top", "free_surface"])
@pytest.mark.parametrize("shape", [(37, 133), (23, 240)], ids=lambda s: "%dx%d" % s)
def test_born_is_the_transpose_partner_of_the_material_gradient(shape, fs):
    c = _case(*shape, fs)
    drec = _born(c)[3:]
    g = _adjoint_source(drec)
    mat, _ = _gradient(c, 0, g)
    _close(_dots(drec, g), _dot(_t(c["dmat"]), mat.grad), 2e-5, "<J dm, g> vs <dm, J^T g>")


@pytest.mark.parametrize("st", [0, 1, 2], ids=["explosive", "fx", "fz"])
@pytest.mark.parametrize("fs", [0, 1], ids=["absorbing_top", "free_surface"])
@pytest.mark.parametrize("shape", [(37, 133), (23, 240)], ids=lambda s: "%dx%d" % s)
def test_born_is_the_transpose_partner_of_the_source_gradient(shape, fs, st):
    c = _case(*shape, fs)
    df = _t(c["df"])
    drec = _born(c, st, dmat=torch.zeros_like(_t(c["mat3"])), df=df)[3:]
    assert all(a.abs().max() > 0 for a in drec)
    g = _adjoint_source(drec)
    _, f = _gradient(c, st, g)
    _close(_dots(drec, g), _dot(df, f.grad), 2e-5, "<J df, g> vs <df, J^T g>")


# ---- 4: linearity and the zero case -------------------------------------------------------------------------------
def test_linearity_and_the_zero_case():
    c = _case(44, 120, 1)
    dm, df = _t(c["dmat"]), _t(c["df"])
    zero = torch.zeros_like(dm)
    for z in _born(c, dmat=zero)[3:]:
        assert torch.equal(z, torch.zeros_like(z))
    one = _stack(_born(c)[3:])
    two = _stack(_born(c, dmat=2.0 * dm)[3:])
    e2 = rel_l2(two, 2.0 * one)
    both = _stack(_born(c, df=df)[3:])
    src = _stack(_born(c, dmat=zero, df=df)[3:])
    es = rel_l2(both, one + src)
    print("born(2 dmat) vs 2 born(dmat): %.3e; born(dmat, df) vs the sum of the parts: %.3e" % (e2, es))
    assert np.abs(src).max() > 0 and np.abs(one).max() > 0
    assert e2 <= 1e-6
    assert es <= 2e-6


# ---- 5: shot chunks and passes ------------------------------------------------------------------------------------
def test_shot_chunks_and_passes_give_the_same_bits(monkeypatch):
    from physicsbasedfwi2_amd import fluid
    c = _case(37, 133, 0)
    pl = fluid.FluidPlan(37, 133, NT, 1, 1, 13, 1, c["fw"], 0)
    one_shot = 4 * NT * pl.layout.snap_step_elems
    pl.close()
    whole = _born(c, 2)
    assert len(whole) == 6 and all(a.abs().max() > 0 for a in whole)
    chunked = _born(c, 2, snapshot_budget=int(1.5 * one_shot))         # holds one shot's snapshots, not two
    for a, b in zip(whole, chunked):
        assert torch.equal(a, b)
    with pytest.raises(fluid.MifwiError):
        _born(c, 2, snapshot_budget=one_shot // 2)
    monkeypatch.setenv("MIFWI_FL_PASS_SHOTS", "1")
    pl = fluid.FluidPlan(37, 133, NT, 3, 1, 13, 1, c["fw"], 0)
    assert pl.pass_sizes()[0] == 1
    pl.close()
    passes = _born(c, 2)
    for a, b in zip(whole, passes):
        assert torch.equal(a, b)


# ---- 6: Gauss-Newton product --------------------------------------------------------------------------------------
def test_gauss_newton_product():
    c = _case(37, 70, 1)
    da, db = _t(c["dmat"]), _t(_case(37, 70, 1, seed=1)["dmat"])
    out_a = _gn(c, da)
    ha, dra = out_a[0], out_a[1:]
    hb = _gn(c, db)[0]
    drec = _born(c)[3:]
    assert len(dra) == 3 and tuple(ha.shape) == (3, 37, 70)
    for a, b in zip(dra, drec):
        assert torch.equal(a, b)
    _close(_dot(da, ha), _dots(drec, drec), 2e-5, "<d, H d> vs |J d|^2")
    ab, ba, scale = _dot(da, hb), _dot(db, ha), (_dot(da, ha) * _dot(db, hb)) ** 0.5
    print("<a, H b> %.9e, <b, H a> %.9e, |diff| / sqrt(<a,Ha><b,Hb>) = %.2e" % (ab, ba, abs(ab - ba) / scale))
    assert abs(ab - ba) <= 2e-5 * scale
    mat, _ = _gradient(c, 0, drec)
    e = rel_l2(ha.cpu().numpy(), mat.grad.double().cpu().numpy())
    h2 = _gn(c, da, weight=lambda x, z, p: (2.0 * x, 2.0 * z, 2.0 * p))[0]
    e2 = rel_l2(h2.cpu().numpy(), 2.0 * ha.double().cpu().numpy())
    print("hv vs propagate + backward(drec): rel-L2 %.3e; doubled weight vs 2 hv: %.3e" % (e, e2))
    assert e <= 2e-5
    assert e2 <= 1e-6            # scaling by 2 is exact in f32: only flush effects remain


# ---- 7: materials_jvp ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fs", [False, True], ids=["absorbing_top", "free_surface"])
def test_materials_jvp_is_the_transpose_of_the_vjp(fs):
    from physicsbasedfwi2_amd import fluid
    c = _case(37, 70, int(fs))
    prm = [torch.tensor(c[k], device=DEV, dtype=torch.float32, requires_grad=True) for k in ("vp", "rho")]
    g = torch.Generator().manual_seed(9)
    d = [(0.01 * torch.randn(p.shape, generator=g)).to(DEV) * p.detach() for p in prm]
    dmat = fluid.materials_jvp(prm[0].detach(), prm[1].detach(), d[0], d[1], c["dt"], c["h"], free_surface=fs)
    assert tuple(dmat.shape) == (3,) + tuple(prm[0].shape) and dmat.is_cuda
    assert bool(torch.isfinite(dmat).all()) and dmat.abs().max() > 0
    if fs:
        assert bool((dmat[0, 0] == 0).all())
    G = torch.randn(dmat.shape, generator=g).to(DEV)
    fluid.materials(*prm, c["dt"], c["h"], free_surface=fs).backward(G)
    _close(_dot(dmat, G), sum(_dot(a, p.grad) for a, p in zip(d, prm)), 2e-5, "<jvp(d), G> vs <d, vjp(G)>")


# ---- 8: refusals --------------------------------------------------------------------------------------------------
def test_refusals():
    from physicsbasedfwi2_amd import fluid
    c = _case(37, 70, 0)
    mat, dm, a = _t(c["mat3"]), _t(c["dmat"]), _args(c)
    with pytest.raises(fluid.MifwiError, match="no CPU fallback"):
        fluid.born(mat.cpu(), dm.cpu(), *[t.cpu() for t in a[:-1]], a[-1])
    with pytest.raises(fluid.MifwiError):
        fluid.born(mat, dm[:, :, :-1], *a)
    with pytest.raises(fluid.MifwiError):
        fluid.gauss_newton_product(mat, dm[:, :-1], *a)
    with pytest.raises(fluid.MifwiError):
        fluid.born(mat, dm, *a, df=a[0][:-1])
    with pytest.raises(fluid.MifwiError):
        fluid.born(mat, dm, *a, source_type="shear")


def test_c_entry_point_refuses_before_any_launch():
    """mifwi_fluid_born itself: null dmat / snap / work and bad ranges return MIFWI_EINVAL before anything is launched."""
    from physicsbasedfwi2_amd import _lib
    from physicsbasedfwi2_amd.fluid import FluidPlan
    lib = _lib.load()
    nz, nx, nt = 44, 60, 8
    buf = torch.zeros(1 << 16, device=DEV)
    cells = torch.zeros(4, device=DEV, dtype=torch.int32)
    P = _lib.ptr
    pl = FluidPlan(nz, nx, nt, 1, 1, 1, 1, 6, 0)

    def call(dmat=buf, snap=buf, work=buf, n0=0, n1=nt, first=0):
        return lib.mifwi_fluid_born(pl.handle, P(buf), P(dmat), P(buf), P(buf), None, P(cells), P(buf), P(cells), P(buf),
                                    P(snap), first, None, None, None, P(work), n0, n1, 0, None)
    try:
        for rc in (call(dmat=None), call(snap=None), call(work=None), call(n0=-1), call(n1=nt + 1), call(n0=5, n1=4),
                   call(n0=2, first=3), call(first=-1)):
            assert rc == -1
        assert call(n0=3, n1=3) == 0                     # an empty range is served: nothing to do
    finally:
        pl.close()
    torch.cuda.synchronize()
    assert not buf.any()
