"""(Vp, Vs, rho) -> staggered material planes on the device (csrc/mifwi_materials.hip) against its definition, the torch
expression of physicsbasedfwi2_amd/elastic.py: the planes bit for bit (same operations in the same order), the chain rule
to fp32 round-off of a different summation order, and against central differences in float64."""
import numpy as np
import pytest
import torch

from physicsbasedfwi2_amd import elastic

pytestmark = pytest.mark.gpu


def _models(nz, nx, seed, water_rows):
    rng = np.random.default_rng(seed)
    vp = 1500.0 + 2500.0 * rng.random((nz, nx))
    vs = vp / (1.6 + 0.4 * rng.random((nz, nx)))
    rho = 1000.0 + 1500.0 * rng.random((nz, nx))
    vs[:water_rows] = 0.0                       # water: mu = 0, the harmonic mean's special case
    vs[nz // 2, nx // 3] = 0.0                  # and an isolated fluid cell
    return [torch.tensor(a, dtype=torch.float32) for a in (vp, vs, rho)]


@pytest.mark.parametrize("nz,nx,fs,water", [(37, 53, False, 0), (100, 300, True, 6), (5, 4, True, 1), (1, 9, False, 0), (9, 1, True, 0)])
def test_fused_materials_match_the_torch_expression(nz, nx, fs, water):
    dev = torch.device("cuda:0")
    dt, h = 2e-3, 20.0
    cpu = [t.clone().requires_grad_(True) for t in _models(nz, nx, 3, water)]
    gpu = [t.detach().to(dev).requires_grad_(True) for t in cpu]
    ref = elastic._staggered_materials_torch(*[t.to(dev) for t in cpu], dt, h, free_surface=fs)      # definition, on the device
    out = elastic.staggered_materials(*gpu, dt, h, free_surface=fs)
    assert out.shape == (5, nz, nx) and out.grad_fn is not None and type(out.grad_fn).__name__.startswith("_MaterialsFn")
    assert torch.equal(out, ref), [float((out[k] - ref[k]).abs().max()) for k in range(5)]
    # the CPU evaluation of the definition (what the oracle compositions of the tests use) agrees to round-off
    ref_cpu = elastic.staggered_materials(*cpu, dt, h, free_surface=fs)
    assert type(ref_cpu.grad_fn).__name__ != "_MaterialsFnBackward"
    assert float((out.detach().cpu() - ref_cpu.detach()).abs().max()) <= 2e-7 * float(ref_cpu.detach().abs().max())
    # chain rule: a random cotangent through both
    rng = np.random.default_rng(5)
    g = torch.tensor(rng.standard_normal((5, nz, nx)), dtype=torch.float32)
    out.backward(g.to(dev))
    ref_cpu.backward(g)
    for a, b, name in zip(gpu, cpu, ("vp", "vs", "rho")):
        err = float((a.grad.cpu() - b.grad).norm() / b.grad.norm())
        assert err <= 2e-6, (name, err)
    # same bits on a second evaluation (gather, no atomics)
    again = [t.detach().clone().requires_grad_(True) for t in gpu]
    elastic.staggered_materials(*again, dt, h, free_surface=fs).backward(g.to(dev))
    assert all(torch.equal(a.grad, b.grad) for a, b in zip(again, gpu))


def test_fused_materials_directional_derivative():
    """<grad, d> from the fused chain rule against a central difference of the float64 definition."""
    dev = torch.device("cuda:0")
    nz, nx, dt, h = 24, 31, 1e-3, 10.0
    m = _models(nz, nx, 11, 3)
    rng = np.random.default_rng(12)
    d = [torch.tensor(rng.standard_normal((nz, nx)), dtype=torch.float64) * s for s in (30.0, 0.0, 20.0)]
    d[1] = torch.tensor(rng.standard_normal((nz, nx)), dtype=torch.float64) * 20.0 * (m[1] > 0)      # water stays water
    c = torch.tensor(rng.standard_normal((5, nz, nx)), dtype=torch.float64)
    f = lambda e: float((elastic.staggered_materials(*[a.double() + e * b for a, b in zip(m, d)], dt, h, free_surface=True) * c).sum())
    eps = 1e-3
    fd = (f(eps) - f(-eps)) / (2 * eps)
    gpu = [t.to(dev).requires_grad_(True) for t in m]
    (elastic.staggered_materials(*gpu, dt, h, free_surface=True) * c.float().to(dev)).sum().backward()
    an = sum(float((a.grad.double().cpu() * b).sum()) for a, b in zip(gpu, d))
    assert abs(an - fd) <= 2e-5 * abs(fd), (an, fd)


@pytest.mark.parametrize("nz,nx,pad", [(174, 500, 20), (33, 47, 6), (5, 3, 0), (1, 7, 4),
                                        (1, 1, 20), (2, 1, 20), (1, 2, 10)])
def test_fused_acoustic_coefficients_match_the_torch_expression(nz, nx, pad):
    """vp -> r = (edge-replicated vp dt/h)^2 of the deepwave-shaped shim: the fused launch against pad, scale, square;
    the chain rule (layer folded into the edge cells) against autograd's, to the round-off of another summation order,
    and against float64 autograd.  On the last three grids every cell is a corner that folds up to (2 pad + 1)^2 layer
    cells: there the bound is derived from the fold count F of each cell - an fp32 sum of F terms is off by at most
    (F - 1) u sum |g|, and x = vp c and the two products after the sum add 3 u, so
        |gvp - gvp_64| <= (F + 3) u sum |g| |2 vp c^2|    (u = 2^-24; first order, +1 for the second-order terms)."""
    from physicsbasedfwi2_amd.compat.deepwave import scalar
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(8)
    vp0 = torch.tensor(1500.0 + 3000.0 * rng.random((nz, nx)), dtype=torch.float32, device=dev)
    c = 1e-3 / 10.0
    a = vp0.clone().requires_grad_(True)
    b = vp0.clone().requires_grad_(True)
    r = scalar._Coefficients.apply(a, pad, c)
    ref = (scalar._EdgePad.apply(b, pad) * c) ** 2
    assert r.shape == (nz + 2 * pad, nx + 2 * pad) and torch.equal(r, ref)
    g = torch.tensor(rng.standard_normal(tuple(r.shape)), dtype=torch.float32, device=dev)
    r.backward(g)
    ref.backward(g)
    if nz * nx > 2:
        # fp32 against fp32 in another summation order; on the folded grids (every cell a corner of up to 1681 terms)
        # that comparison is made through the float64 bound below instead
        assert float((a.grad - b.grad).norm() / b.grad.norm()) <= 1e-6
    # float64 autograd of the same expression, with the constant the kernel receives (an fp32 c)
    c64 = float(np.float32(c))
    v64 = vp0.double().cpu()

    def pull(cot):
        v = v64.clone().requires_grad_(True)
        ((scalar._EdgePad.apply(v, pad) * c64) ** 2).backward(cot)
        return v.grad

    want = pull(g.double().cpu())
    size = pull(g.double().cpu().abs())                                   # sum |g| |2 vp c^2|
    ones = torch.ones(nz, nx, dtype=torch.float64, requires_grad=True)
    scalar._EdgePad.apply(ones, pad).backward(torch.ones(tuple(r.shape), dtype=torch.float64))
    fold = ones.grad                                                      # F: layer cells folded into each cell
    assert float(fold.sum()) == r.numel()
    err = (a.grad.double().cpu() - want).abs()
    assert bool((err <= (fold + 3) * 2.0 ** -24 * size).all()), float((err / size).max())
    a2 = vp0.clone().requires_grad_(True)
    scalar._Coefficients.apply(a2, pad, c).backward(g)
    assert torch.equal(a2.grad, a.grad)


@pytest.mark.parametrize("mode", [elastic.PARAM_VELOCITY, elastic.PARAM_IMPEDANCE, elastic.PARAM_LAME])
def test_gradient_parametrization_is_the_jacobian_of_the_change_of_variables(mode):
    """mifwi_elastic_gradient_parametrization (DENISE's INVMAT1, models/networks.py:11025) against float64 autograd of
    the change of variables itself: (Zp, Zs, rho) -> (Zp / rho, Zs / rho, rho) and (lambda, mu, rho) ->
    (sqrt((lambda + 2 mu) / rho), sqrt(mu / rho), rho), a random cotangent pulled back.  Water cells (Vs = 0) take no
    Vs term in the Lame form (the kernel's convention: the shear gradient is 0 there anyway - mu_xz = 0)."""
    dev = torch.device("cuda:0")
    vp, vs, rho = _models(41, 67, 11, 5)
    rng = np.random.default_rng(12)
    g = [torch.tensor(rng.standard_normal(vp.shape), dtype=torch.float32) for _ in range(3)]
    g[1][vs == 0] = 0.0
    out = elastic.gradient_parametrization([t.to(dev) for t in (vp, vs, rho)], [t.to(dev) for t in g], mode)
    P, Q, R = (t.double() for t in (vp, vs, rho))
    if mode == elastic.PARAM_VELOCITY:
        new = [P.clone().requires_grad_(True), Q.clone().requires_grad_(True), R.clone().requires_grad_(True)]
        old = new
    elif mode == elastic.PARAM_IMPEDANCE:
        new = [(R * P).requires_grad_(True), (R * Q).requires_grad_(True), R.clone().requires_grad_(True)]
        old = [new[0] / new[2], new[1] / new[2], new[2]]
    else:
        mu = R * Q * Q
        new = [(R * P * P - 2 * mu).requires_grad_(True), mu.requires_grad_(True), R.clone().requires_grad_(True)]
        wet = Q == 0
        shear = torch.where(wet, torch.zeros_like(mu), torch.sqrt(torch.where(wet, torch.ones_like(mu), new[1]) / new[2]))
        old = [torch.sqrt((new[0] + 2 * new[1]) / new[2]), shear, new[2]]
    sum((o * c.double()).sum() for o, c in zip(old, g)).backward()
    for k in range(3):
        want = new[k].grad
        got = out[k].cpu().double()
        assert float((got - want).abs().max()) <= 4e-6 * float(want.abs().max()), (mode, k)
    if mode == elastic.PARAM_VELOCITY:
        assert all(torch.equal(o.cpu(), c) for o, c in zip(out, g))


@pytest.mark.parametrize("mode", [elastic.PARAM_VELOCITY, elastic.PARAM_IMPEDANCE, elastic.PARAM_LAME])
def test_gradient_parametrization_at_zero_velocity_and_zero_density_cells(mode):
    """reparam_vjp divides by rho, rho Vp and 2 rho Vp: isolated Vp = 0, rho = 0 and Vp = Vs = rho = 0 cells (the DENISE
    shim's VPLOWERLIM is 0) give finite gradients, with the convention of include/mifwi.h - a term whose divisor is zero
    contributes 0.  Against float64 autograd of the change of variables written with that convention; the documented
    aliasing of outputs and inputs through the C entry point gives the same bits."""
    from physicsbasedfwi2_amd import _lib
    dev = torch.device("cuda:0")
    nz, nx = 23, 37
    vp, vs, rho = _models(nz, nx, 13, 3)
    cells = {"vp": (6, 7), "rho": (9, 11), "all": (15, 20), "water vp": (1, 30)}
    vp[cells["vp"]] = 0.0
    rho[cells["rho"]] = 0.0
    vp[cells["all"]] = vs[cells["all"]] = rho[cells["all"]] = 0.0
    vp[cells["water vp"]] = 0.0                                        # Vs = 0 there already
    rng = np.random.default_rng(14)
    g = [torch.tensor(rng.standard_normal(vp.shape), dtype=torch.float32) for _ in range(3)]
    g[1][vs == 0] = 0.0
    prm = [t.to(dev) for t in (vp, vs, rho)]
    gd = [t.to(dev) for t in g]
    out = elastic.gradient_parametrization(prm, gd, mode)
    assert all(bool(torch.isfinite(o).all()) for o in out), mode
    P, Q, R = (t.double() for t in (vp, vs, rho))
    one = torch.ones_like(P)
    if mode == elastic.PARAM_VELOCITY:
        new = [P.clone().requires_grad_(True), Q.clone().requires_grad_(True), R.clone().requires_grad_(True)]
        old = new
    elif mode == elastic.PARAM_IMPEDANCE:
        new = [(R * P).requires_grad_(True), (R * Q).requires_grad_(True), R.clone().requires_grad_(True)]
        dry = R == 0
        safe = torch.where(dry, one, new[2])
        old = [torch.where(dry, 0 * one, new[0] / safe), torch.where(dry, 0 * one, new[1] / safe), new[2]]
    else:
        mu = R * Q * Q
        new = [(R * P * P - 2 * mu).requires_grad_(True), mu.requires_grad_(True), R.clone().requires_grad_(True)]
        no_p = (P == 0) | (R == 0)
        no_s = (Q == 0) | (R == 0)
        old = [torch.where(no_p, 0 * one, torch.sqrt(torch.where(no_p, one, new[0] + 2 * new[1]) / torch.where(no_p, one, new[2]))),
               torch.where(no_s, 0 * one, torch.sqrt(torch.where(no_s, one, new[1]) / torch.where(no_s, one, new[2]))),
               new[2]]
    sum((o * c.double()).sum() for o, c in zip(old, g)).backward()
    for k in range(3):
        want = new[k].grad
        got = out[k].cpu().double()
        assert bool(torch.isfinite(want).all())
        assert float((got - want).abs().max()) <= 4e-6 * float(want.abs().max()), (mode, k)
    if mode != elastic.PARAM_VELOCITY:
        for name in ("rho", "all"):                                    # rho = 0: the rho gradient passes unchanged
            assert float(out[0][cells[name]]) == 0.0 and float(out[1][cells[name]]) == 0.0, (mode, name)
            assert float(out[2][cells[name]]) == float(g[2][cells[name]]), (mode, name)
    if mode == elastic.PARAM_LAME:
        for name in ("vp", "water vp"):                                # Vp = 0: no lambda gradient
            assert float(out[0][cells[name]]) == 0.0, name
    # out_* = the gradient inputs themselves: the same bits
    lib = _lib.load()
    al = [t.clone() for t in gd]
    with torch.cuda.device(dev):
        _lib.check(lib.mifwi_elastic_gradient_parametrization(
            0, int(mode), *[_lib.ptr(t) for t in prm], *[_lib.ptr(t) for t in al], *[_lib.ptr(t) for t in al],
            vp.numel(), torch.cuda.current_stream().cuda_stream))
    assert all(torch.equal(a, o) for a, o in zip(al, out)), mode
