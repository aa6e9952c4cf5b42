"""What the VTI propagator (physicsbasedfwi2_amd.vti, mifwi_vti_*) has of its own on the GPU: Thomsen's kinematics on the
kernels, PHYSICS = 3 of the pyapi_denise shim and the refusals of the C entry points.  The isotropic limit and the parity with
the float64 reference keep their names here and run the checks of tests/psv_media.py that the viscoelastic medium runs too
(shapes A ... D, bounds and what was measured: there and in tests/test_psv_media_gpu.py, which has Born and the driver
forms), as does the run of A and B at forced tile widths."""
import ctypes

import numpy as np
import pytest
import torch

import psv_media as M
import psv_reference as R
from cases import rel_l2
from psv_media import CASES, TOL_TRACE, dev as _dev

pytestmark = pytest.mark.gpu
VTI = M.MEDIA["vti"]


@pytest.fixture(autouse=True)
def _no_fallback():
    yield from M.no_fallback()


# ---- the isotropic limit at mat level, anisotropic parity: the shared checks --------------------------------------------
@pytest.mark.parametrize("order", [2, 4])
@pytest.mark.parametrize("form", ["default", "per_step"])
@pytest.mark.parametrize("name", list(CASES))
def test_isotropic_limit_is_the_elastic_propagator(monkeypatch, name, form, order):
    M.check_limit_is_the_elastic_propagator(VTI, monkeypatch, name, form, order)


@pytest.mark.parametrize("order", [2, 4])
@pytest.mark.parametrize("name", list(CASES))
def test_anisotropic_traces_and_gradients_match_the_reference(name, order):
    M.check_traces_and_gradients_match_the_reference(VTI, name, order)


@pytest.mark.parametrize("order", [2, 4])
@pytest.mark.parametrize("name,lx", [("B", 32), ("B", 64), ("A", 64)])
def test_forced_tile_width_matches_the_reference(monkeypatch, name, lx, order):
    """B (38 groups) at 32 lanes: two tile columns, the second with 6 live lanes; at 64: one partial column; A: 15 of 64"""
    M.check_forced_width(VTI, monkeypatch, name, lx, order)


# ---- the physics pin on the kernels --------------------------------------------------------------------------------
def test_kernels_travel_at_the_thomsen_velocities():
    from physicsbasedfwi2_amd import vti

    def run(mat6, pz, px, f, sc, sw, rc, rw):
        out = vti.propagate(_dev(mat6), _dev(f), _dev(pz), _dev(px), _dev(sc), _dev(sw), _dev(rc), _dev(rw), 0)
        return [a.double().cpu().numpy() for a in out]
    R.pin_check(run)


# ---- the pyapi_denise shim ----------------------------------------------------------------------------------------
def _denise(tmp_path, physics):
    import physicsbasedfwi2_amd.compat.pyapi_denise as api
    rng = np.random.default_rng(3)
    nz, nx, dx = 48, 70, 20.0
    vp = (1800 + 1200 * rng.random((nz, nx))).astype(np.float32)
    vs = (vp / np.sqrt(3)).astype(np.float32)
    rho = (1900 + 300 * rng.random((nz, nx))).astype(np.float32)
    vs[:8] = 0; vp[:8] = 1500; rho[:8] = 1000
    d = api.Denise("/nonexistent", verbose=0)
    d.save_folder = str(tmp_path)
    d.PHYSICS, d.ITERMAX = physics, 1
    d.TIME, d.DT, d.FREE_SURF, d.FW, d.FPML, d.DAMPING = 0.3, 0.0015, 1, 8, 5.0, 1500.0
    xsrc = np.array([400.0, 1000.0])
    src = api.Sources(xsrc, 40.0 * xsrc / xsrc, 8.0)
    xrec = np.arange(300.0, 1100.0 + dx, 40.0)
    rec = api.Receivers(xrec, 460.0 * (xrec / xrec))
    z, x = np.meshgrid(np.arange(nz) / nz, np.arange(nx) / nx, indexing="ij")
    eps = (0.12 + 0.1 * np.sin(5 * z + 3 * x)).astype(np.float32)
    dl = (0.03 + 0.1 * np.cos(4 * z - 2 * x)).astype(np.float32)
    eps[:8] = 0; dl[:8] = 0
    return api, d, (vp, vs, rho, eps, dl), dx, src, rec


def test_shim_physics3_isotropic_limit_gradients_and_refusals(tmp_path, monkeypatch):
    from physicsbasedfwi2_amd import misfit, vti
    monkeypatch.chdir(tmp_path)
    api, d, (vp, vs, rho, eps, dl), dx, src, rec = _denise(tmp_path, 3)
    model = api.Model(np.flipud(vp), np.flipud(vs), np.flipud(rho), dx)
    with pytest.raises(api.MifwiError, match="set_thomsen"):
        d.forward(model, src, rec)
    # epsilon = delta = 0: the PHYSICS = 1 seismograms
    d.set_thomsen(np.zeros_like(vp), np.zeros_like(vp))
    zx, zy = d.forward(model, src, rec)
    _, d1, _, _, _, _ = _denise(tmp_path, 1)
    ex, ey = d1.forward(model, src, rec)
    assert np.abs(ex).max() > 0 and np.abs(ey).max() > 0
    e = rel_l2(np.stack([zx, zy]), np.stack([ex, ey]))
    print("PHYSICS 3 with epsilon = delta = 0 vs PHYSICS 1: rel-L2 %.2e" % e)
    assert e <= TOL_TRACE
    # an anisotropic model: observed data from a perturbed one, five gradients
    d.set_thomsen(np.flipud(eps * 1.2), np.flipud(dl * 0.8))
    ox, oy = d.forward(api.Model(np.flipud(vp * 1.03), np.flipud(vs * 0.98), np.flipud(rho), dx), src, rec)
    assert rel_l2(np.stack([ox, oy]), np.stack([ex, ey])) > 0.02
    d.set_observed(np.transpose(ox, (0, 2, 1)), np.transpose(oy, (0, 2, 1)))
    d.set_thomsen(np.flipud(eps), np.flipud(dl))
    loss = d.grad(model, src, rec)
    g_rho, g_vp, g_vs = (np.flipud(a) for a in d.get_fwi_gradients(["seis"]))
    g_eps, g_dl = (np.flipud(a) for a in d.get_thomsen_gradients())
    for a in (g_rho, g_vp, g_vs, g_eps, g_dl):
        assert a.shape == vp.shape and np.isfinite(a).all() and np.abs(a).max() > 0
    # the same by hand: vti.materials + vti.propagate + misfit.l2_half
    dev, h, dt, nt, g, f, pz, px, fw, fsurf = d._setup(model, src, rec)
    prm = [torch.tensor(a.copy(), device=dev, requires_grad=True) for a in (vp, vs, rho, eps, dl)]
    mat = vti.materials(*prm, dt, h, free_surface=fsurf)
    vx, vy = vti.propagate(mat, f.to(dev), pz, px, g["sc"], g["sw"], g["rc"], g["rw"], fw, free_surface=fsurf,
                           fd_order=int(d.FD_ORDER))
    tx, ty = (torch.tensor(np.ascontiguousarray(np.transpose(a, (2, 0, 1))), device=dev) for a in (ox, oy))
    hand = misfit.l2_half(vy, ty) + misfit.l2_half(vx, tx)
    hand.backward()
    assert abs(float(hand.detach()) - loss) <= 1e-6 * abs(loss)
    for name, got, p in (("vp", g_vp, prm[0]), ("vs", g_vs, prm[1]), ("rho", g_rho, prm[2]), ("epsilon", g_eps, prm[3]),
                         ("delta", g_dl, prm[4])):
        e = rel_l2(got, p.grad.cpu().numpy())
        print("shim gradient %s vs by hand: rel-L2 %.2e" % (name, e))
        assert e <= 1e-6, name
    # the depth taper reaches all five
    d.SWS_TAPER_GRAD_HOR, d.GRADT1, d.GRADT2, d.GRADT3, d.GRADT4 = 1, 10, 14, 40, 44
    d.grad(model, src, rec)
    for a in list(d.get_fwi_gradients(["seis"])) + list(d.get_thomsen_gradients()):
        a = np.flipud(a)
        assert not a[:10].any() and not a[44:].any() and np.abs(a[14:40]).max() > 0
    d.SWS_TAPER_GRAD_HOR = 0
    # refusals
    for attr, bad, good in (("INVMAT1", 2, 1), ("EPRECOND", 1, 0), ("SEISMO", 2, 1), ("SEISMO", 4, 1), ("QUELLTYPB", 4, 1),
                            ("acoustic_kernels", "fluid", "elastic")):
        setattr(d, attr, bad)
        with pytest.raises(api.MifwiError):
            d.grad(model, src, rec)
        setattr(d, attr, good)
    d.set_thomsen(np.zeros((3, 3)), np.zeros((3, 3)))
    with pytest.raises(api.MifwiError):
        d.forward(model, src, rec)
    with pytest.raises(api.MifwiError):
        d.set_thomsen(np.zeros((3, 3)), np.zeros((3, 4)))
    d.set_thomsen(None, None)
    with pytest.raises(api.MifwiError, match="set_thomsen"):
        d.grad(model, src, rec)
    with pytest.raises(api.MifwiError):
        d1.get_thomsen_gradients()


# ---- the C entry points ---------------------------------------------------------------------------------------------
def test_c_entry_points_refuse_nulls_bad_ranges_and_born_with_a_force_source():
    from physicsbasedfwi2_amd import _lib, vti
    lib = _lib.load()
    EINVAL = -1
    h = ctypes.c_void_p()
    for bad in (dict(ntap=2), dict(nz=0), dict(nshot=0), dict(source_type=3), dict(fd_order=3), dict(pml_width=-1),
                dict(nz=12, nx=12, pml_width=8)):
        kw = dict(nz=20, nx=24, nt=10, nshot=2, nsrc=1, nrec=3, ntap=1, pml_width=4, free_surface=0, shots_per_group=0,
                  source_type=0, fd_order=4)
        kw.update(bad)
        assert lib.mifwi_vti_plan_create(ctypes.byref(h), 0, ctypes.byref(_lib.VtiDesc(**kw))) == EINVAL, bad
    assert lib.mifwi_vti_plan_create(None, 0, None) == EINVAL
    assert lib.mifwi_vti_plan_layout(None, None) == EINVAL and lib.mifwi_vti_plan_pass_sizes(None, None, None) == EINVAL
    dev = torch.device("cuda:0")
    for st in (0, 1):
        plan = vti.VtiPlan(20, 24, 10, 2, 1, 3, 1, 4, 0, source_type=st)
        lay = plan.layout
        assert plan.pass_sizes() == (2, lay.ngroups) and plan.cluster_slabs() == 0
        z = lambda *s: torch.zeros(*s, device=dev)
        mat, pz, px, f = z(6, 20, lay.gp), z(6, 20), z(6, lay.gp), z(10, 2, 1)
        cell, w = torch.zeros(2, 3, 1, dtype=torch.int32, device=dev), z(2, 3, 1)
        scell, sw = torch.zeros(2, 1, 1, dtype=torch.int32, device=dev), z(2, 1, 1)
        rec, snap = z(10, 2, 3), z(10, lay.snap_step_elems)
        work = z(max(lay.work_forward_elems, lay.work_backward_elems))
        P = _lib.ptr
        geo = (P(scell), P(sw), P(cell), P(w))
        fwd = lambda m=P(mat), b=0, e=10, wk=P(work): lib.mifwi_vti_forward(
            plan.handle, m, P(pz), P(px), P(f), *geo, P(rec), P(rec), P(snap), wk, b, e, _lib.ZERO_STATE, None)
        assert fwd(m=None) == EINVAL and fwd(wk=None) == EINVAL
        assert fwd(b=-1) == EINVAL and fwd(e=11) == EINVAL and fwd(b=5, e=4) == EINVAL
        assert lib.mifwi_vti_forward(None, P(mat), P(pz), P(px), P(f), *geo, P(rec), P(rec), P(snap), P(work), 0, 10, 1,
                                     None) == EINVAL
        bwd = lambda s=P(snap), hi=9, lo=0, gx=P(rec): lib.mifwi_vti_backward(
            plan.handle, P(mat), P(pz), P(px), *geo, gx, P(rec), s, 0, P(mat), None, P(work), hi, lo,
            _lib.ZERO_STATE | _lib.FINALIZE, None)
        assert bwd(s=None) == EINVAL and bwd(gx=None) == EINVAL and bwd(hi=10) == EINVAL and bwd(lo=-1) == EINVAL
        born = lambda dm=P(mat), s=P(snap), b=0, e=10: lib.mifwi_vti_born(
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
