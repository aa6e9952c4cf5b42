"""The viscoelastic propagator's host side without a GPU: the yardstick (tests/psv_reference.py) against its VTI form
in the elastic limit (itself pinned to the fp64 C oracle), against the attenuation law of a standard linear solid and
against its own central differences; ``visco.materials`` / ``materials_jvp`` / ``max_velocity`` / ``relaxation`` on CPU
float64; the C ABI of the ``mifwi_visco_*`` structs."""
import ctypes

import numpy as np
import pytest
import torch

import psv_reference as R
from cases import elastic_case, rel_l2
from psv_media import check_struct_layouts, seeded_model

RELAX = (0.9, 0.1)             # any pair inside (0, 1): with planes 5-7 zero it must not matter


# ---- 1: the elastic limit of the reference ---------------------------------------------------------------------------
@pytest.mark.parametrize("order", [2, 4])
@pytest.mark.parametrize("fs", [False, True], ids=["absorbing_top", "free_surface"])
def test_reference_is_the_vti_reference_in_the_elastic_limit(fs, order):
    """Planes 5-7 zero: the memory variables stay 0 and every stress update is the VTI form's in its isotropic limit,
    which tests/test_vti_host.py pins to the fp64 oracle.  Same operations in the same order: the bound is 1e-16 rel-L2
    (measured 0)."""
    c = elastic_case(seed=4, free_surface=fs)
    geo = (c["sc"], c["sw"], c["rc"], c["rw"])
    mat8 = np.concatenate([c["mat"], np.zeros((3,) + c["mat"].shape[1:])])
    mat6 = np.concatenate([c["mat"], c["mat"][1:2]])
    with torch.no_grad():
        got = R.forward(mat8, c["pz"], c["px"], c["f"], *geo, "visco", RELAX, free_surface=c["fs"], fd_order=order)
        want = R.forward(mat6, c["pz"], c["px"], c["f"], *geo, "vti", free_surface=c["fs"], fd_order=order)
    got, want = np.stack([a.numpy() for a in got]), np.stack([a.numpy() for a in want])
    err = rel_l2(got, want)
    print("visco reference (planes 5-7 zero) vs vti reference (isotropic): rel-L2 %.2e" % err)
    assert np.abs(want[0]).max() > 0 and np.abs(want[1]).max() > 0
    assert err <= 1e-16


# ---- 2: attenuation -----------------------------------------------------------------------------------------------------
ATT = dict(n=(121, 201), nt=600, h=10.0, dt=1e-3, f0=15.0, src=(60, 50), offsets=(30, 80), vp=2000.0, vs=1100.0, rho=2000.0,
           qp=30.0, qs=25.0)
ATT_BOUND = 5e-3


def _att_traces(qp, qs):
    from oracle import helpers as H
    from physicsbasedfwi2_amd import visco
    a = ATT
    nz, nx = a["n"]
    full = lambda v: np.full((nz, nx), float(v))
    mat = R.visco_mat8(full(a["vp"]), full(a["vs"]), full(a["rho"]), full(qp), full(qs), a["f0"], a["f0"], a["dt"], a["h"])
    tz, tx = np.zeros((6, nz)), np.zeros((6, nx))
    tz[R.PK] = tz[R.PKH] = tx[R.PK] = tx[R.PKH] = 1.0
    t = np.arange(a["nt"]) * a["dt"] - 1.2 / a["f0"]
    w = (np.pi * a["f0"] * t) ** 2
    f = ((1 - 2 * w) * np.exp(-w))[:, None, None] * 1e6
    sz, sx = a["src"]
    sc, sw = H.cell_taps(np.array([[sz]]), np.array([[sx]]), nx)
    rc, rw = H.cell_taps(np.array([[sz, sz]]), np.array([[sx + o for o in a["offsets"]]]), nx)
    with torch.no_grad():
        vx, _ = R.forward(mat, tz, tx, f, sc, sw, rc, rw, "visco", visco.relaxation(a["f0"], a["dt"]))
    return vx.numpy()[:, 0, :]


def test_reference_attenuates_as_the_standard_linear_solid():
    """Homogeneous full space (121 x 201 cells of 10 m, no layer: the window of 600 steps ends before the first edge
    reflection reaches a receiver), explosive 15 Hz Ricker, vx receivers 300 m and 800 m from the source on its row;
    Qp = 30, f_relax = f_ref = 15 Hz, against the lossless run at the same vp.  At f_ref the amplitude-spectrum ratio
    (visco / elastic at r2) / (visco / elastic at r1) is exp(-pi f (r2 - r1) / (Q(f) vp)) with the SLS's own Q(w).
    Measured: 0.68278 against 0.68384, a relative deviation of 1.55e-3 (first-order attenuation law, far-field spreading,
    time discretisation of the memory variable); the bound is 5e-3, about 3 times that.  tau or tau_sigma wrong by a factor
    of 2 either way moves the prediction by 6.9e-2 ... 4.3e-1 relative: the same bound rejects each of them."""
    a = ATT
    v, e = _att_traces(a["qp"], a["qs"]), _att_traces(np.inf, np.inf)
    assert np.abs(e[-5:]).max() <= 2e-3 * np.abs(e).max()                  # the wavelet has passed both receivers
    ph = np.exp(-2j * np.pi * a["f0"] * a["dt"] * np.arange(a["nt"]))[:, None]
    av, ae = np.abs((v * ph).sum(0)), np.abs((e * ph).sum(0))
    measured = (av[1] / ae[1]) / (av[0] / ae[0])
    dr = (a["offsets"][1] - a["offsets"][0]) * a["h"]
    law = lambda f_relax, tau: np.exp(-np.pi * a["f0"] * dr / (R.sls_q(a["f0"], f_relax, tau) * a["vp"]))
    tau = 2.0 / a["qp"]
    dev = abs(measured / law(a["f0"], tau) - 1.0)
    print("amplitude ratio at f_ref: measured %.5f, the SLS law %.5f, relative deviation %.2e (bound %.1e)"
          % (measured, law(a["f0"], tau), dev, ATT_BOUND))
    assert measured < 0.75                                                # it attenuates for real
    assert dev <= ATT_BOUND
    for f_relax, t in ((a["f0"], 2 * tau), (a["f0"], tau / 2), (2 * a["f0"], tau), (a["f0"] / 2, tau)):
        wrong = abs(measured / law(f_relax, t) - 1.0)
        print("  with f_relax %.1f, tau %.4f the law would be off by %.2e" % (f_relax, t, wrong))
        assert wrong > ATT_BOUND


# ---- 3: visco.materials and its companions on CPU float64 ----------------------------------------------------------------
def _model(*a, **kw):
    """vp, vs, rho, qp in [20, 200], qs in [10, 100]"""
    return seeded_model((20, 180), (10, 90), *a, **kw)


def test_materials_without_attenuation_are_the_elastic_planes():
    from physicsbasedfwi2_amd import elastic, visco
    vp, vs, rho, _, _ = _model(9, 11)
    inf = torch.full_like(vp, float("inf"))
    for fs in (False, True):
        m = visco.materials(vp, vs, rho, inf, inf, 12.0, 9.0, 1e-3, 10.0, free_surface=fs)
        assert m.shape == (8, 9, 11) and m.dtype == torch.float64
        assert torch.equal(m[:5], elastic._staggered_materials_torch(vp, vs, rho, 1e-3, 10.0, free_surface=fs))
        assert not m[5:].any()


def test_materials_obey_the_standard_linear_solid():
    """Re M(w_ref) = rho v^2 (the velocities are those AT f_ref, DENISE's convention), Q(w_ref) of the planes is the model's
    Q up to the SLS's own Q(w) law, the sxz node averages as the elastic one, the free-surface row is in effective form."""
    from physicsbasedfwi2_amd import elastic, visco
    vp, vs, rho, qp, qs = _model(9, 11, seed=2)
    dt, h, f_ref, f_relax = 1e-3, 10.0, 12.0, 9.0
    s = dt / h
    m = visco.materials(vp, vs, rho, qp, qs, f_ref, f_relax, dt, h)
    x2 = (f_ref / f_relax) ** 2
    sd = x2 / (1 + x2)
    pi_r = m[1] - m[6]                                        # lam2mu_u - R1 = pi_r
    re_m = pi_r + sd * m[6]                                   # Re M(w) = M_r (1 + s tau)
    assert float((re_m / (rho * s) / (vp * vp) - 1).abs().max()) <= 1e-12
    taup = m[6] / pi_r
    assert float((taup * qp / 2 - 1).abs().max()) <= 1e-12
    q_ref = torch.tensor(R.sls_q(f_ref, f_relax, taup.numpy()))
    im_m = pi_r * taup * (f_ref / f_relax) / (1 + x2)          # Im M(w) = M_r tau w tau_sigma / (1 + w^2 tau_sigma^2)
    assert float((re_m / im_m / q_ref - 1).abs().max()) <= 1e-12
    # R2 = R1 - 2 mu_r tau_s, lam_u = lam2mu_u - 2 mu_u on the collocated node
    taus = 2.0 / qs
    mu_r = rho * vs * vs / (1 + sd * taus)
    scale = float(m[1].abs().max())
    assert float((m[5] - (m[6] - 2 * mu_r * taus * s)).abs().max()) <= 1e-12 * scale
    assert float((m[0] - (m[1] - 2 * mu_r * (1 + taus) * s)).abs().max()) <= 1e-12 * scale
    # planes 3, 4: the elastic bits; sxz node: zero in and next to the water, harmonic mu_r times (1 + / times) mean tau_s
    m5 = elastic._staggered_materials_torch(vp, vs, rho, dt, h)
    assert torch.equal(m[3], m5[3]) and torch.equal(m[4], m5[4])
    assert not m[2][:1].any() and not m[7][:1].any() and bool((m[2][1:] > 0).all()) and bool((m[7][1:] > 0).all())
    j, i = 4, 5
    corners = [(j, i), (j, i + 1), (j + 1, i), (j + 1, i + 1)]
    mh = 4.0 / sum(1.0 / mu_r[c] for c in corners)
    ta = sum(taus[c] for c in corners) / 4.0
    assert abs(float(m[2][j, i]) / float(mh * (1 + ta) * s) - 1) <= 1e-12
    assert abs(float(m[7][j, i]) / float(mh * ta * s) - 1) <= 1e-12
    # a homogeneous solid: the sxz node carries Re mu(w_ref) = rho vs^2
    one = torch.ones(4, 4, dtype=torch.float64)
    mh8 = visco.materials(2000 * one, 1100 * one, 2000 * one, 40 * one, 30 * one, f_ref, f_relax, dt, h)
    assert float(((mh8[2] - mh8[7] + sd * mh8[7]) / (2000 * s) / 1100 ** 2 - 1).abs().max()) <= 1e-12
    # free surface: row 0 in effective form, from the row's earlier values; the other rows untouched
    mf = visco.materials(vp, vs, rho, qp, qs, f_ref, f_relax, dt, h, free_surface=True)
    assert not mf[0][0].any() and not mf[5][0].any()
    assert float((mf[6][0] - (m[6][0] - m[5][0] * m[0][0] / m[1][0])).abs().max()) <= 1e-12 * scale
    assert float((mf[1][0] - (m[1][0] - m[0][0] ** 2 / m[1][0])).abs().max()) <= 1e-12 * scale
    assert torch.equal(mf[:, 1:], m[:, 1:]) and torch.equal(mf[[2, 3, 4, 7]], m[[2, 3, 4, 7]])


def test_max_velocity_is_the_unrelaxed_p_velocity_and_relaxation_the_crank_nicolson_pair():
    from physicsbasedfwi2_amd import visco
    vp, _, rho, qp, _ = _model(6, 7, seed=1)
    f_ref, f_relax, dt, h = 10.0, 14.0, 1e-3, 10.0
    m = visco.materials(vp, torch.zeros_like(vp), rho, qp, qp, f_ref, f_relax, dt, h)
    want = float(torch.sqrt(m[1] / (dt / h) / rho).max())
    assert abs(visco.max_velocity(vp, qp, f_ref, f_relax) / want - 1) <= 1e-12
    assert visco.max_velocity(vp, qp, f_ref, f_relax) > float(vp.max())
    assert visco.max_velocity(vp, torch.full_like(vp, float("inf")), f_ref, f_relax) == float(vp.max())
    a, b = visco.relaxation(f_relax, dt)
    eta = 2 * np.pi * f_relax * dt
    assert a == (2 - eta) / (2 + eta) and b == 2 * eta / (2 + eta) and abs(a + b - 1) <= 1e-15


@pytest.mark.parametrize("fs", [False, True])
def test_materials_jvp_is_the_directional_derivative_and_the_transpose_of_the_vjp(fs):
    from physicsbasedfwi2_amd import visco
    prm = _model(6, 7, seed=5)
    rng = np.random.default_rng(6)
    tan = [torch.tensor(rng.standard_normal(p.shape)) * s for p, s in zip(prm, (10.0, 10.0, 10.0, 1.0, 1.0))]
    tan[1] = tan[1] * (prm[1] > 0)
    kw = dict(f_ref=12.0, f_relax=9.0, dt=1e-3, h=10.0, free_surface=fs)
    d = visco.materials_jvp(*prm, *tan, **kw)
    e = 1e-4
    p = visco.materials(*[a + e * b for a, b in zip(prm, tan)], **kw)
    q = visco.materials(*[a - e * b for a, b in zip(prm, tan)], **kw)
    err = rel_l2(d.numpy(), ((p - q) / (2 * e)).numpy())
    print("materials_jvp vs central difference: rel-L2 %.2e" % err)
    assert d.shape == (8, 6, 7) and err <= 1e-7
    # <J t, g> = <t, J^T g> with J^T by autograd
    lead = [a.clone().requires_grad_(True) for a in prm]
    g = torch.tensor(rng.standard_normal(d.shape)) * d.abs().amax(dim=(1, 2), keepdim=True).clamp_min(1e-300).reciprocal()
    (visco.materials(*lead, **kw) * g).sum().backward()
    lhs, rhs = float((d * g).sum()), float(sum((a.grad * t).sum() for a, t in zip(lead, tan)))
    print("<J t, g> = %.12e, <t, J^T g> = %.12e" % (lhs, rhs))
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), abs(rhs))


def test_materials_and_relaxation_refuse_what_has_no_meaning():
    from physicsbasedfwi2_amd import visco
    from physicsbasedfwi2_amd._lib import MifwiError
    vp, vs, rho, qp, qs = _model()
    ok = dict(f_ref=12.0, f_relax=9.0, dt=1e-3, h=10.0)
    visco.materials(vp, vs, rho, qp, qs, **ok)
    for bad in (0.0, -5.0, float("nan")):
        q = qp.clone()
        q[2, 3] = bad
        with pytest.raises(MifwiError, match="qp"):
            visco.materials(vp, vs, rho, q, qs, **ok)
        with pytest.raises(MifwiError, match="qs"):
            visco.materials(vp, vs, rho, qp, q, **ok)
        with pytest.raises(MifwiError, match="qp"):
            visco.materials_jvp(vp, vs, rho, q, qs, vp, vs, rho, qp, qs, **ok)
    for f_relax in (0.0, -1.0):
        with pytest.raises(MifwiError, match="f_relax"):
            visco.materials(vp, vs, rho, qp, qs, 12.0, f_relax, 1e-3, 10.0)
        with pytest.raises(MifwiError, match="f_relax"):
            visco.relaxation(f_relax, 1e-3)
        with pytest.raises(MifwiError, match="f_relax"):
            visco.max_velocity(vp, qp, 12.0, f_relax)
    with pytest.raises(MifwiError, match="eta"):
        visco.relaxation(400.0, 1e-3)                        # eta = 2.51
    with pytest.raises(MifwiError, match="eta"):
        visco.materials(vp, vs, rho, qp, qs, 12.0, 400.0, 1e-3, 10.0)
    with pytest.raises(MifwiError, match="f_ref"):
        visco.materials(vp, vs, rho, qp, qs, 0.0, 9.0, 1e-3, 10.0)


# ---- 4: the reference's own adjoint -------------------------------------------------------------------------------------
@pytest.mark.parametrize("fs", [False, True], ids=["absorbing_top", "free_surface"])
def test_reference_gradient_is_its_central_difference(fs):
    """Autograd through the float64 recursion against a central difference of the same recursion, in one seeded random
    direction of all eight planes and of f.  The difference's own error: the step is 1e-3 of a 1 % perturbation, 1e-5 of
    each plane, so truncation is ~ 1e-10 of the first derivative and cancellation ~ 1e-16 / 1e-5; the bound is 1e-7."""
    from physicsbasedfwi2_amd import visco
    c = elastic_case(seed=9, nz=30, nx=40, nt=70, nrec=5, free_surface=fs)
    rng = np.random.default_rng(3)
    nz, nx = c["vp"].shape
    qp, qs = 20 + 60 * rng.random((nz, nx)), 10 + 40 * rng.random((nz, nx))
    mat8 = R.visco_mat8(c["vp"], c["vs"], c["rho"], qp, qs, 8.0, 8.0, c["dt"], c["h"], free_surface=fs)
    relax = visco.relaxation(8.0, c["dt"])
    geo = (c["sc"], c["sw"], c["rc"], c["rw"])
    kw = dict(free_surface=c["fs"], fd_order=4)
    def g_of(rvx, rvz):
        r = np.random.default_rng(4)
        return [r.standard_normal(a.shape) * np.abs(a).max() for a in (rvx, rvz)]
    rvx, rvz, gm, gf = R.gradients(mat8, c["pz"], c["px"], c["f"], *geo, g_of, None, "visco", relax, **kw)
    g = g_of(rvx, rvz)
    dmat = 0.01 * rng.standard_normal(mat8.shape) * mat8
    df = 0.01 * rng.standard_normal(c["f"].shape) * np.abs(c["f"]).max()
    assert all(np.abs(dmat[k]).max() > 0 and np.abs(gm[k]).max() > 0 for k in range(8))
    for what, dm, dff, lhs in (("mat", dmat, None, float((gm * dmat).sum())), ("f", 0 * dmat, df, float((gf * df).sum()))):
        J = R.jvp(mat8, dm, c["pz"], c["px"], c["f"], dff, *geo, "visco", relax, eps=1e-3, **kw)
        rhs = float((J[0] * g[0]).sum() + (J[1] * g[1]).sum())
        err = abs(lhs - rhs) / max(abs(lhs), abs(rhs))
        print("<grad_%s, d> = %.12e, <g, J d> by central difference = %.12e, relative difference %.2e" % (what, lhs, rhs, err))
        assert err <= 1e-7


# ---- 5: ABI ------------------------------------------------------------------------------------------------------------
def test_visco_struct_layouts_match_header(tmp_path):
    from physicsbasedfwi2_amd import _lib
    structs = {"mifwi_visco_desc": _lib.ViscoDesc, "mifwi_visco_layout": _lib.ViscoLayout}
    check_struct_layouts(structs, tmp_path)
    assert ctypes.sizeof(_lib.ViscoDesc) == 14 * 4
    assert [n for n, _ in _lib.ViscoDesc._fields_] == [n for n, _ in _lib.VtiDesc._fields_] + ["relax_a", "relax_b"]
    # the elastic and VTI descriptors and the version stay
    assert ctypes.sizeof(_lib.ElasticDesc) == 14 * 4 and ctypes.sizeof(_lib.VtiDesc) == 12 * 4
    assert _lib.load().mifwi_version() == 7


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-device error path")
def test_visco_fails_loudly_without_a_device():
    from physicsbasedfwi2_amd import _lib, visco
    from physicsbasedfwi2_amd._lib import MifwiError
    lib = _lib.load()
    h = ctypes.c_void_p()
    d = _lib.ViscoDesc(8, 8, 4, 1, 1, 1, 1, 0, 0, 0, 0, 4, 0.9, 0.1)
    rc = lib.mifwi_visco_plan_create(ctypes.byref(h), 0, ctypes.byref(d))
    assert rc == -2 and b"no CPU fallback" in lib.mifwi_last_error()
    assert lib.mifwi_visco_plan_create(None, 0, ctypes.byref(d)) == -1
    for a, b in ((0.0, 0.1), (1.0, 0.1), (0.9, 0.0), (0.9, 1.5), (float("nan"), 0.1)):
        bad = _lib.ViscoDesc(8, 8, 4, 1, 1, 1, 1, 0, 0, 0, 0, 4, a, b)
        assert lib.mifwi_visco_plan_create(ctypes.byref(h), 0, ctypes.byref(bad)) == -1 and b"relax" in lib.mifwi_last_error()
    assert lib.mifwi_visco_plan_cluster_slabs(None, 0) == 0
    one = torch.zeros(1, 1, 1, dtype=torch.int32)
    with pytest.raises(MifwiError):
        visco.propagate(torch.ones(8, 8, 8), torch.zeros(4, 1, 1), torch.zeros(6, 8), torch.zeros(6, 8), one,
                        torch.ones(1, 1, 1), one, torch.ones(1, 1, 1), 0, 10.0, 1e-3)
