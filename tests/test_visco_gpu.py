"""What the viscoelastic propagator (physicsbasedfwi2_amd.visco, mifwi_visco_*) has of its own on the GPU: L = 1 of the
pyapi_denise shim and the refusals of the C entry points, the elastic ones' of the other media's plans included.  The
elastic limit and the parity with the float64 reference keep their names here and run the checks of tests/psv_media.py that
the VTI medium runs too (shapes A ... D, bounds and what was measured: there and in tests/test_psv_media_gpu.py, which has
Born and the driver forms), as does the run of A and B at forced tile widths.
Measured on the MI355X: the shim against the by-hand composition and L = 1 with Q = inf against L = 0: the same bits."""
import ctypes

import numpy as np
import pytest
import torch

import psv_media as M
from cases import rel_l2
from psv_media import CASES, TOL_TRACE

pytestmark = pytest.mark.gpu
VISCO = M.MEDIA["visco"]


@pytest.fixture(autouse=True)
def _no_fallback():
    yield from M.no_fallback()


# ---- the elastic limit at mat level (the per-step kernels' only), attenuating parity: the shared checks ------------------
@pytest.mark.parametrize("order", [2, 4])
@pytest.mark.parametrize("name", list(CASES))
def test_elastic_limit_is_the_elastic_propagator(monkeypatch, name, order):
    M.check_limit_is_the_elastic_propagator(VISCO, monkeypatch, name, "per_step", order)


@pytest.mark.parametrize("order", [2, 4])
@pytest.mark.parametrize("name", list(CASES))
def test_attenuating_traces_and_gradients_match_the_reference(name, order):
    M.check_traces_and_gradients_match_the_reference(VISCO, name, order)


@pytest.mark.parametrize("order", [2, 4])
@pytest.mark.parametrize("name,lx", [("B", 32), ("B", 64), ("A", 64)])
def test_forced_tile_width_matches_the_reference(monkeypatch, name, lx, order):
    """B (38 groups) at 32 lanes: two tile columns, the second with 6 live lanes; at 64: one partial column; A: 15 of 64"""
    M.check_forced_width(VISCO, monkeypatch, name, lx, order)


# ---- the pyapi_denise shim ------------------------------------------------------------------------------------------------
def _denise(tmp_path, L):
    import physicsbasedfwi2_amd.compat.pyapi_denise as api
    rng = np.random.default_rng(3)
    nz, nx, dx = 48, 70, 20.0
    vp = (1800 + 1200 * rng.random((nz, nx))).astype(np.float32)
    vs = (vp / np.sqrt(3)).astype(np.float32)
    rho = (1900 + 300 * rng.random((nz, nx))).astype(np.float32)
    vs[:8] = 0; vp[:8] = 1500; rho[:8] = 1000
    d = api.Denise("/nonexistent", verbose=0)
    d.save_folder = str(tmp_path)
    d.PHYSICS, d.ITERMAX, d.L, d.FL1 = 1, 1, L, 8.0
    d.TIME, d.DT, d.FREE_SURF, d.FW, d.FPML, d.DAMPING = 0.3, 0.0015, 1, 8, 5.0, 1500.0
    xsrc = np.array([400.0, 1000.0])
    src = api.Sources(xsrc, 40.0 * xsrc / xsrc, 8.0)
    xrec = np.arange(300.0, 1100.0 + dx, 40.0)
    rec = api.Receivers(xrec, 460.0 * (xrec / xrec))
    z, x = np.meshgrid(np.arange(nz) / nz, np.arange(nx) / nx, indexing="ij")
    qp = (60 + 35 * np.sin(5 * z + 3 * x)).astype(np.float32)
    qs = (40 + 25 * np.cos(4 * z - 2 * x)).astype(np.float32)
    qp[:8] = 1000.0
    return api, d, (vp, vs, rho, qp, qs), dx, src, rec


def test_shim_attenuation_by_hand_gradients_lossless_limit_and_refusals(tmp_path, monkeypatch):
    from physicsbasedfwi2_amd import elastic, misfit, visco
    monkeypatch.chdir(tmp_path)
    api, d, (vp, vs, rho, qp, qs), dx, src, rec = _denise(tmp_path, 1)
    model = api.Model(np.flipud(vp), np.flipud(vs), np.flipud(rho), dx)
    # every refusal comes before the device is touched: with no device named, _setup would ask torch for the current one
    def current_device():
        raise AssertionError("the device was touched")
    with monkeypatch.context() as m:
        m.setattr(torch.cuda, "current_device", current_device)
        with pytest.raises(api.MifwiError, match="set_attenuation"):
            d.forward(model, src, rec)                                              # missing Q arrays
        d.set_attenuation(np.flipud(qp), np.flipud(qs))
        d.set_observed(np.zeros((2, 200, 21)), np.zeros((2, 200, 21)))
        for attr, bad, good in (("PHYSICS", 2, 1), ("PHYSICS", 3, 1), ("EPRECOND", 1, 0), ("SEISMO", 2, 1), ("SEISMO", 4, 1),
                                ("QUELLTYPB", 4, 1)):
            setattr(d, attr, bad)
            with pytest.raises(api.MifwiError):
                d.forward(model, src, rec)
            with pytest.raises(api.MifwiError):
                d.grad(model, src, rec)
            setattr(d, attr, good)
        d.set_attenuation(np.ones((3, 3)), np.ones((3, 3)))
        with pytest.raises(api.MifwiError, match="set_attenuation"):
            d.forward(model, src, rec)
        with pytest.raises(api.MifwiError):
            d.set_attenuation(np.ones((3, 3)), np.ones((3, 4)))
        with pytest.raises(api.MifwiError):
            d.set_attenuation(np.ones((3, 3)), None)
        for bad in (2, 3, -1, "1"):
            with pytest.raises(api.MifwiError, match="L="):
                d.L = bad
        assert d.L == 1
        with pytest.raises(api.MifwiError):
            d.get_attenuation_gradients()
    # L = 1 against visco.propagate fed by hand
    d.set_attenuation(np.flipud(qp), np.flipud(qs))
    sx, sy = d.forward(model, src, rec)
    dev, h, dt, nt, g, f, pz, px, fw, fsurf = d._setup(model, src, rec)
    f_ref = 8.0                                                  # F_REF = None: the first source's centre frequency
    hand = lambda *prm: visco.propagate(visco.materials(*prm, f_ref, d.FL1, dt, h, free_surface=fsurf), f.to(dev), pz, px,
                                        g["sc"], g["sw"], g["rc"], g["rw"], fw, d.FL1, dt, free_surface=fsurf,
                                        fd_order=int(d.FD_ORDER))
    with torch.no_grad():
        hx, hy = hand(*[torch.tensor(a.copy(), device=dev) for a in (vp, vs, rho, qp, qs)])
    want = np.stack([hx.permute(1, 2, 0).cpu().numpy(), hy.permute(1, 2, 0).cpu().numpy()])
    e = rel_l2(np.stack([sx, sy]), want)
    print("shim L = 1 vs visco.propagate by hand: rel-L2 %.2e" % e)
    assert np.abs(want).max() > 0 and e <= TOL_TRACE
    # the CFL limit is taken at the unrelaxed velocity
    vmax = visco.max_velocity(vp, qp, f_ref, d.FL1)
    assert vmax > float(vp.max())
    from physicsbasedfwi2_amd import profiles
    d.DT = 0.5 * (profiles.elastic_cfl_limit(h, vmax, int(d.FD_ORDER)) + profiles.elastic_cfl_limit(h, float(vp.max()), int(d.FD_ORDER)))
    with pytest.raises(api.MifwiError, match="stability"):
        d.forward(model, src, rec)
    d.DT = 0.0015
    # Q = inf: the L = 0 seismograms
    inf = np.full_like(vp, np.inf)
    d.set_attenuation(inf, inf)
    ix, iy = d.forward(model, src, rec)
    _, d0, _, _, _, _ = _denise(tmp_path, 0)
    ex, ey = d0.forward(model, src, rec)
    assert np.abs(ex).max() > 0 and np.abs(ey).max() > 0
    e = rel_l2(np.stack([ix, iy]), np.stack([ex, ey]))
    print("L = 1 with Q = inf vs L = 0: rel-L2 %.2e, attenuating vs L = 0: %.2e" % (e, rel_l2(np.stack([sx, sy]), np.stack([ex, ey]))))
    assert e <= TOL_TRACE
    assert rel_l2(np.stack([sx, sy]), np.stack([ex, ey])) > 0.01
    # gradients for INVMAT1 = 1, 2, 3 against autograd through visco.materials (and the change of variables)
    d.set_attenuation(np.flipud(qp * 1.2), np.flipud(qs * 0.8))
    ox, oy = d.forward(api.Model(np.flipud(vp * 1.03), np.flipud(vs * 0.98), np.flipud(rho), dx), src, rec)
    d.set_observed(np.transpose(ox, (0, 2, 1)), np.transpose(oy, (0, 2, 1)))
    d.set_attenuation(np.flipud(qp), np.flipud(qs))
    prm = [torch.tensor(a.copy(), device=dev, requires_grad=True) for a in (vp, vs, rho, qp, qs)]
    vx, vy = hand(*prm)
    tx, ty = (torch.tensor(np.ascontiguousarray(np.transpose(a, (2, 0, 1))), device=dev) for a in (ox, oy))
    by_hand = misfit.l2_half(vy, ty) + misfit.l2_half(vx, tx)
    by_hand.backward()
    for invmat in (1, 2, 3):
        d.INVMAT1 = invmat
        loss = d.grad(model, src, rec)
        assert abs(float(by_hand.detach()) - loss) <= 1e-6 * abs(loss)
        g_rho, g_vp, g_vs = (np.flipud(a) for a in d.get_fwi_gradients(["seis"]))
        g_qp, g_qs = (np.flipud(a) for a in d.get_attenuation_gradients())
        w3 = [p.grad for p in prm[:3]]
        if invmat != 1:
            w3 = elastic.gradient_parametrization([p.detach() for p in prm[:3]], w3, invmat)
        for nm, got, want in (("first", g_vp, w3[0]), ("second", g_vs, w3[1]), ("rho", g_rho, w3[2]), ("qp", g_qp, prm[3].grad),
                              ("qs", g_qs, prm[4].grad)):
            assert got.shape == vp.shape and np.isfinite(got).all() and np.abs(got).max() > 0, nm
            e = rel_l2(got, want.cpu().numpy())
            print("INVMAT1 %d shim gradient %s vs by hand: rel-L2 %.2e" % (invmat, nm, e))
            assert e <= 1e-6, (invmat, nm)
    d.INVMAT1 = 1
    with pytest.raises(api.MifwiError):
        d0.get_attenuation_gradients()
    # L = 0 changes nothing: the Q arrays are ignored
    d0.set_attenuation(np.flipud(qp), np.flipud(qs))
    zx, zy = d0.forward(model, src, rec)
    assert np.array_equal(zx, ex) and np.array_equal(zy, ey)


# ---- the C entry points -----------------------------------------------------------------------------------------------------
def test_c_entry_points_refuse_nulls_bad_ranges_and_born_with_a_force_source():
    from physicsbasedfwi2_amd import _lib, visco
    lib = _lib.load()
    EINVAL = -1
    h = ctypes.c_void_p()
    for bad in (dict(ntap=2), dict(nz=0), dict(nshot=0), dict(source_type=3), dict(fd_order=3), dict(pml_width=-1),
                dict(nz=12, nx=12, pml_width=8), dict(relax_a=0.0), dict(relax_a=1.0), dict(relax_b=0.0), dict(relax_b=2.0),
                dict(relax_a=float("nan"))):
        kw = dict(nz=20, nx=24, nt=10, nshot=2, nsrc=1, nrec=3, ntap=1, pml_width=4, free_surface=0, shots_per_group=0,
                  source_type=0, fd_order=4, relax_a=0.9, relax_b=0.1)
        kw.update(bad)
        assert lib.mifwi_visco_plan_create(ctypes.byref(h), 0, ctypes.byref(_lib.ViscoDesc(**kw))) == EINVAL, bad
    assert lib.mifwi_visco_plan_create(None, 0, None) == EINVAL
    assert lib.mifwi_visco_plan_layout(None, None) == EINVAL and lib.mifwi_visco_plan_pass_sizes(None, None, None) == EINVAL
    dev = torch.device("cuda:0")
    for st in (0, 1):
        plan = visco.ViscoPlan(20, 24, 10, 2, 1, 3, 1, 4, 0, 0.9, 0.1, source_type=st)
        lay = plan.layout
        assert plan.pass_sizes() == (2, lay.ngroups) and plan.cluster_slabs() == 0
        z = lambda *s: torch.zeros(*s, device=dev)
        mat, pz, px, f = z(8, 20, lay.gp), z(6, 20), z(6, lay.gp), z(10, 2, 1)
        cell, w = torch.zeros(2, 3, 1, dtype=torch.int32, device=dev), z(2, 3, 1)
        scell, sw = torch.zeros(2, 1, 1, dtype=torch.int32, device=dev), z(2, 1, 1)
        rec, snap = z(10, 2, 3), z(10, lay.snap_step_elems)
        work = z(max(lay.work_forward_elems, lay.work_backward_elems))
        P = _lib.ptr
        geo = (P(scell), P(sw), P(cell), P(w))
        fwd = lambda m=P(mat), b=0, e=10, wk=P(work): lib.mifwi_visco_forward(
            plan.handle, m, P(pz), P(px), P(f), *geo, P(rec), P(rec), P(snap), wk, b, e, _lib.ZERO_STATE, None)
        assert fwd(m=None) == EINVAL and fwd(wk=None) == EINVAL
        assert fwd(b=-1) == EINVAL and fwd(e=11) == EINVAL and fwd(b=5, e=4) == EINVAL
        assert lib.mifwi_visco_forward(None, P(mat), P(pz), P(px), P(f), *geo, P(rec), P(rec), P(snap), P(work), 0, 10, 1,
                                       None) == EINVAL
        bwd = lambda s=P(snap), hi=9, lo=0, gx=P(rec): lib.mifwi_visco_backward(
            plan.handle, P(mat), P(pz), P(px), *geo, gx, P(rec), s, 0, P(mat), None, P(work), hi, lo,
            _lib.ZERO_STATE | _lib.FINALIZE, None)
        assert bwd(s=None) == EINVAL and bwd(gx=None) == EINVAL and bwd(hi=10) == EINVAL and bwd(lo=-1) == EINVAL
        born = lambda dm=P(mat), s=P(snap), b=0, e=10: lib.mifwi_visco_born(
            plan.handle, P(mat), dm, P(pz), P(px), None, *geo, s, 0, P(rec), P(rec), P(work), b, e, _lib.ZERO_STATE, None)
        assert born(dm=None) == EINVAL and born(s=None) == EINVAL and born(e=11) == EINVAL
        if st == 1:
            assert born() == EINVAL and b"point-force" in lib.mifwi_last_error()
            assert fwd() == 0 and bwd() == 0                          # a force source is refused by Born alone
            torch.cuda.synchronize()
        else:
            assert fwd() == 0 and bwd() == 0 and born() == 0          # the valid calls pass
            torch.cuda.synchronize()
        plan.close()
    # a handle of another medium is refused, not run on eight planes
    from physicsbasedfwi2_amd import vti
    other = vti.VtiPlan(20, 24, 10, 2, 1, 3, 1, 4, 0)
    assert lib.mifwi_visco_forward(other.handle, None, None, None, None, None, None, None, None, None, None, None, None, 0, 10,
                                   0, None) == EINVAL and b"mifwi_visco_plan_create" in lib.mifwi_last_error()
    other.close()


def test_elastic_entry_points_refuse_the_plans_of_the_other_media():
    """mifwi_elastic_forward / _backward / _born would run six- or eight-plane kernels on what their caller allocated as
    five planes: a VTI or viscoelastic handle is refused before anything is read or launched (all arguments null)."""
    from physicsbasedfwi2_amd import _lib, elastic, visco, vti
    lib = _lib.load()
    EINVAL, N = -1, None
    for other in (vti.VtiPlan(20, 24, 10, 2, 1, 3, 1, 4, 0), visco.ViscoPlan(20, 24, 10, 2, 1, 3, 1, 4, 0, 0.9, 0.1)):
        calls = (lambda: lib.mifwi_elastic_forward(other.handle, *[N] * 12, 0, 10, 0, N),
                 lambda: lib.mifwi_elastic_backward(other.handle, *[N] * 10, 0, N, N, N, 9, 0, 0, N),
                 lambda: lib.mifwi_elastic_born(other.handle, *[N] * 10, 0, N, N, N, 0, 10, 0, N))
        for call in calls:
            assert call() == EINVAL and b"not created by mifwi_elastic_plan_create" in lib.mifwi_last_error()
        other.close()
    # its own handle still passes
    dev = torch.device("cuda:0")
    plan = elastic.ElasticPlan(20, 24, 10, 2, 1, 3, 1, 4, 0)
    lay = plan.layout
    z = lambda *s: torch.zeros(*s, device=dev)
    mat, pz, px, f, rec, work = z(5, 20, lay.gp), z(6, 20), z(6, lay.gp), z(10, 2, 1), z(10, 2, 3), z(lay.work_forward_elems)
    scell, sw = torch.zeros(2, 1, 1, dtype=torch.int32, device=dev), z(2, 1, 1)
    cell, w = torch.zeros(2, 3, 1, dtype=torch.int32, device=dev), z(2, 3, 1)
    P = _lib.ptr
    assert lib.mifwi_elastic_forward(plan.handle, P(mat), P(pz), P(px), P(f), P(scell), P(sw), P(cell), P(w), P(rec), P(rec),
                                     None, P(work), 0, 10, _lib.ZERO_STATE, None) == 0
    torch.cuda.synchronize()
    plan.close()
