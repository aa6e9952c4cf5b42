"""The TTI propagator (physicsbasedfwi2_amd.tti, mifwi_tti_*) on the GPU: the isotropic and the VTI limit, parity with the
float64 reference of tests/tti_reference.py on the shapes A ... D of tests/psv_media.py (at most 37 x 150, 3 shots, 120
steps), forced tile widths, four-tap points and force sources, Born and Gauss-Newton products, time checkpoints, the 45
degree pin on the kernels, PHYSICS = 4 of the pyapi_denise shim and the refusals of the C entry points.  Bounds: traces
within TOL_TRACE, every gradient within max(TOL_SUM, 4 E_iso), E_iso measured in the same run on the isotropic kernels -
the project's bounds for a medium on these kernels (psv_media.check_traces_and_gradients_match_the_reference).
On all these cases the only fluid is the water layer, so the mask of the scheme is constant along every row: fluid blocks in
the solid, the other snapshot layout and the free-surface forms are in tests/test_tti_edges_gpu.py, Born on all eight cases
and the driver forms in tests/test_psv_media_gpu.py, random configurations in tests/test_psv_fuzz_gpu.py.
Four-tap points with force sources, measured: fx and fz, orders 2 and 4, absorbing top: traces 8.8e-8 ... 1.3e-7, gradients
1.3e-7 ... 1.2e-6 (c11, fx at order 4); under a free surface: traces 7.4e-8 ... 2.0e-7, gradients 8.1e-8 ... 1.3e-6 (c11, fx
at order 4); E_iso <= 7.7e-7."""
import ctypes

import numpy as np
import pytest
import torch

import psv_media as M
import psv_reference as R
import tti_reference as T
from cases import rel_l2
from psv_media import CASES, TOL_SUM, TOL_TRACE, dev as _dev

pytestmark = pytest.mark.gpu
TTI, VTI = T.TTI, M.MEDIA["vti"]
_cache = {}


@pytest.fixture(autouse=True)
def _no_fallback():
    yield from M.no_fallback()


# ---- the two limits -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [2, 4])
@pytest.mark.parametrize("form", ["default", "per_step"])
@pytest.mark.parametrize("name", list(CASES))
def test_isotropic_limit_is_the_elastic_propagator(monkeypatch, name, form, order):
    M.check_limit_is_the_elastic_propagator(TTI, monkeypatch, name, form, order)


def _ref_no_coupling(name, order):
    """The reference on the case's planes with c15 = c35 = 0, once per case"""
    key = (name, order)
    if key not in _cache:
        c = M.case(TTI, name)
        mat = T.no_coupling(c["matm"])
        out = R.gradients(mat, c["pz"], c["px"], c["f"], *M.geo(c), M.g_of, None, "tti", free_surface=c["fs"], fd_order=order)
        _cache[key] = mat, M.g_of(out[0], out[1]), out[2]
    return _cache[key]


@pytest.mark.parametrize("order", [2, 4])
@pytest.mark.parametrize("name", list(CASES))
def test_vti_limit_is_the_vti_propagator(name, order):
    """c15 = c35 = 0 on the case's rotated planes: the traces of vti.propagate on planes 0-5 bit for bit, their gradients
    within TOL_SUM of VTI's.  The gradients of c15 and c35 do not vanish at zero coupling; they are held to the reference
    within max(TOL_SUM, 4 E_iso[L]) with E_iso[L] measured here on the isotropic kernels."""
    c = M.case(TTI, name)
    mat, g, want = _ref_no_coupling(name, order)
    tvx, tvz, tg, tgf = M.run(TTI, c, mat, order, g)
    vvx, vvz, vg, vgf = M.run(VTI, c, mat[:6], order, g)
    assert float(tvx.abs().max()) > 0 and float(tvz.abs().max()) > 0
    assert torch.equal(tvx, vvx) and torch.equal(tvz, vvz)
    errs = [rel_l2(tg[k], vg[k]) for k in range(6)] + [rel_l2(tgf, vgf)]
    print("tti(c15 = c35 = 0) vs vti gradients rel-L2 %s" % ["%.1e" % e for e in errs])
    assert max(errs) <= TOL_SUM
    iso = M.ref(TTI, name, order, "matlim")
    eg = M.run(None, c, c["mat"], order, iso["g"])[2]
    tol = max(TOL_SUM, 4 * rel_l2(eg[0], iso["planes"][0]))
    for k in (6, 7):
        e = rel_l2(tg[k], want[k])
        print("gradient %s at zero coupling vs reference: rel-L2 %.2e (bound %.2e)" % (TTI.planes[k], e, tol))
        assert np.abs(want[k]).max() > 0
        assert e <= tol


# ---- parity with the reference ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [2, 4])
@pytest.mark.parametrize("name", list(CASES))
def test_tilted_traces_and_gradients_match_the_reference(name, order):
    M.check_traces_and_gradients_match_the_reference(TTI, name, order)


@pytest.mark.parametrize("order", [2, 4])
@pytest.mark.parametrize("name", [n for n in CASES if n != "A_fs"])
def test_the_tilt_moves_the_traces(name, order):
    """The reference with the tilt field against the reference at theta = 0 (the VTI planes of the same Thomsen fields):
    more than 1 % on some live shot.  Not A_fs: its one live shot is shot and recorded in the water row."""
    tilted, flat = M.ref(TTI, name, order, "matm"), M.ref(VTI, name, order, "matm")
    a, b = np.stack([tilted["rvx"], tilted["rvz"]]), np.stack([flat["rvx"], flat["rvz"]])
    moved = [rel_l2(a[:, :, s], b[:, :, s]) for s in M.live_shots(a, 1e-3)]
    print("tilt field vs theta = 0, %s order %d: rel-L2 of the live shots %s" % (name, order, ["%.2e" % v for v in moved]))
    assert max(moved) > 0.01


@pytest.mark.parametrize("order", [2, 4])
@pytest.mark.parametrize("name,lx", [("B", 32), ("B", 64), ("A", 64)])
def test_forced_tile_width_matches_the_reference(monkeypatch, name, lx, order):
    """The strain and stress launches honour MIFWI_EL_LX as the V launch does: B (38 groups) at 32 lanes: two tile columns,
    the second with 6 live lanes; at 64: one partial column; A: 15 of 64"""
    M.check_forced_width(TTI, monkeypatch, name, lx, order)


@pytest.mark.parametrize("order", [2, 4])
@pytest.mark.parametrize("fs", [False, True], ids=["absorbing_top", "free_surface"])
@pytest.mark.parametrize("st", [1, 2])
def test_four_tap_points_and_force_sources(st, fs, order):
    """Under the free surface shot 0 is recorded on the buried line of shot 1: on row 0 its own source's injection is 1e5
    times everything else the case records (psv_media._config)"""
    cfg = dict(source_type=st, ntap=4, free_surface=True, surface_receivers=False) if fs else dict(source_type=st, ntap=4)
    M.check_traces_and_gradients_match_the_reference(TTI, cfg, order)


# ---- Born, Gauss-Newton -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [2, 4])
@pytest.mark.parametrize("name", ["A", "C"])
def test_born_is_the_directional_derivative_of_the_reference(name, order):
    c = M.case(TTI, name)
    want = M.ref_jvp(TTI, name, order)
    _, _, dvx, dvz = M.born(TTI, c, order)
    err = rel_l2(M.pair(dvx, dvz), want)
    print("tti.born vs central difference of the reference, %s order %d: rel-L2 %.3e" % (name, order, err))
    assert np.abs(want).max() > 0
    assert err <= TOL_TRACE


@pytest.mark.parametrize("name", ["A", "C"])
def test_born_dot_products_gauss_newton_and_the_force_refusal(name):
    from physicsbasedfwi2_amd import tti
    from physicsbasedfwi2_amd._lib import MifwiError
    c = M.case(TTI, name)
    order = 4
    dev, dot, close = M.dev, M.dot, M.close
    rvx, rvz, mvx, mvz = M.born(TTI, c, order)
    pvx, pvz = M.run(TTI, c, c["matm"], order)
    assert torch.equal(rvx, pvx) and torch.equal(rvz, pvz)                         # the background traces
    g = M.g_of(rvx.cpu().numpy(), rvz.cpu().numpy())
    _, _, gm, gf = M.run(TTI, c, c["matm"], order, g)
    close(dot(mvx, dev(g[0])) + dot(mvz, dev(g[1])), float((gm * c["dmat"]).sum()), TOL_SUM, "<J dm, g> vs <dm, J^T g>")
    # the two planes of the tilt alone (a sum of terms of both signs: held to TOL_SUM of their absolute sum)
    only = np.array(c["dmat"])
    only[:6] = 0.0
    _, _, qvx, qvz = M.born(TTI, c, order, dmat=dev(only))
    assert float(qvx.abs().max()) > 0
    lhs, rhs = dot(qvx, dev(g[0])) + dot(qvz, dev(g[1])), float((gm[6:] * only[6:]).sum())
    size = float(np.abs(gm[6:] * only[6:]).sum())
    print("<J dc, g> = %.9e, <dc, J^T g> = %.9e, sum |terms| = %.3e, |diff| / sum = %.2e" % (lhs, rhs, size, abs(lhs - rhs) / size))
    assert abs(lhs - rhs) <= TOL_SUM * size
    # Gauss-Newton: Born followed by the adjoint
    a = M.args(c, dev(c["matm"]))
    kw = dict(free_surface=bool(c["fs"]), fd_order=order)
    hv, hvx, hvz = tti.gauss_newton_product(a[0], dev(c["dmat"]), *a[1:], **kw)
    assert torch.equal(hvx, mvx) and torch.equal(hvz, mvz)
    _, _, jtj, _ = M.run(TTI, c, c["matm"], order, [mvx.double().cpu().numpy(), mvz.double().cpu().numpy()], need_f=False)
    e = rel_l2(hv.double().cpu().numpy(), jtj)
    print("gauss_newton_product vs Born followed by the adjoint: rel-L2 %.2e" % e)
    assert hv.shape == (8,) + c["vp"].shape and np.abs(jtj).max() > 0 and e <= TOL_SUM
    close(dot(hv, dev(c["dmat"])), dot(mvx, mvx) + dot(mvz, mvz), TOL_SUM, "<H a, a> vs |J a|^2")
    with pytest.raises(MifwiError, match="explosive"):
        tti.born(a[0], dev(c["dmat"]), *a[1:], source_type="fx", **kw)
    with pytest.raises(MifwiError, match="pseudo"):
        tti.propagate(*a, pseudo_hessian=object())


# ---- driver forms -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("segments", [3, 4])
@pytest.mark.parametrize("name", ["A", "B"])
def test_time_checkpoints_and_repeats_give_the_same_bits(name, segments):
    """Three and four segments: the driver gives a segment's snapshots and as much again to the checkpoints, so a budget
    that holds half the run holds all of it and two segments never occur (_driver.segment_length).  A segment's re-run
    writes its strains into its snapshot planes as the resident run did, the forward pass of a checkpointed run into the
    work planes: the same values either way, and the adjoint reads the same planes in the same order: traces and
    gradients the same bits."""
    c = M.case(TTI, name)
    g = M.ref(TTI, name, 4, "matm")["g"]
    host = lambda t: np.asarray(t.cpu() if torch.is_tensor(t) else t)
    base = M.run(TTI, c, c["matm"], 4, g)
    if segments == 3:
        for a, b in zip(base, M.run(TTI, c, c["matm"], 4, g)):                     # a repeated call
            assert np.array_equal(host(a), host(b))
        for gs in (1, 2):                                                          # shots per gradient accumulator
            r = M.run(TTI, c, c["matm"], 4, g, shots_per_group=gs)
            assert torch.equal(r[0], base[0]) and torch.equal(r[1], base[1])
            assert max(rel_l2(r[2][k], base[2][k]) for k in range(8)) <= TOL_SUM
    seg = M.run(TTI, c, c["matm"], 4, g, snapshot_budget=M.segment_budget(TTI, c, segments))
    for a, b in zip(base, seg):
        assert np.array_equal(host(a), host(b))


# ---- the physics pin on the kernels -------------------------------------------------------------------------------------
@pytest.mark.parametrize("theta_deg", [45, -45])
def test_kernels_travel_along_and_across_the_tilted_axis(theta_deg):
    from physicsbasedfwi2_amd import tti

    def run(mat8, pz, px, f, sc, sw, rc, rw):
        out = tti.propagate(_dev(mat8), _dev(f), _dev(pz), _dev(px), _dev(sc), _dev(sw), _dev(rc), _dev(rw), 0)
        return out[0].double().cpu().numpy()
    T.pin_check(run, theta_deg)


# ---- the pyapi_denise shim ----------------------------------------------------------------------------------------------
# the 48 x 70 set-up of tests/test_vti_gpu.py
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


def test_shim_physics4_zero_tilt_gradients_and_refusals(tmp_path, monkeypatch):
    from physicsbasedfwi2_amd import misfit, tti
    monkeypatch.chdir(tmp_path)
    api, d, (vp, vs, rho, eps, dl), dx, src, rec = _denise(tmp_path, 4)
    nz, nx = vp.shape
    z, x = np.meshgrid(np.arange(nz) / nz, np.arange(nx) / nx, indexing="ij")
    th = (0.5 * np.sin(4 * z - 3 * x)).astype(np.float32)
    th[:8] = 0
    model = api.Model(np.flipud(vp), np.flipud(vs), np.flipud(rho), dx)
    with pytest.raises(api.MifwiError, match="set_thomsen"):
        d.forward(model, src, rec)
    d.set_thomsen(np.flipud(eps), np.flipud(dl))
    with pytest.raises(api.MifwiError, match="theta"):                  # PHYSICS = 4 without a tilt: before device work
        d.forward(model, src, rec)
    # theta = 0: the PHYSICS = 3 seismograms
    d.set_thomsen(np.flipud(eps), np.flipud(dl), np.zeros_like(vp))
    zx, zy = d.forward(model, src, rec)
    _, d3, _, _, _, _ = _denise(tmp_path, 3)
    d3.set_thomsen(np.flipud(eps), np.flipud(dl), np.zeros_like(vp))    # a zero tilt is no tilt
    ex, ey = d3.forward(model, src, rec)
    assert np.abs(ex).max() > 0 and np.abs(ey).max() > 0
    e = rel_l2(np.stack([zx, zy]), np.stack([ex, ey]))
    print("PHYSICS 4 with theta = 0 vs PHYSICS 3: rel-L2 %.2e" % e)
    assert e <= TOL_TRACE
    d3.set_thomsen(np.flipud(eps), np.flipud(dl), np.flipud(th))
    with pytest.raises(api.MifwiError, match="PHYSICS = 4"):
        d3.forward(model, src, rec)
    # a tilted model: observed data from a perturbed one, six gradients
    d.set_thomsen(np.flipud(eps * 1.2), np.flipud(dl * 0.8), np.flipud(th * 0.7))
    ox, oy = d.forward(api.Model(np.flipud(vp * 1.03), np.flipud(vs * 0.98), np.flipud(rho), dx), src, rec)
    assert rel_l2(np.stack([ox, oy]), np.stack([ex, ey])) > 0.02
    d.set_observed(np.transpose(ox, (0, 2, 1)), np.transpose(oy, (0, 2, 1)))
    d.set_thomsen(np.flipud(eps), np.flipud(dl))
    with pytest.raises(api.MifwiError, match="theta"):                  # grad() too, once it has its observed data
        d.grad(model, src, rec)
    d.set_thomsen(np.flipud(eps), np.flipud(dl), np.flipud(th))
    loss = d.grad(model, src, rec)
    g_rho, g_vp, g_vs = (np.flipud(a) for a in d.get_fwi_gradients(["seis"]))
    g_eps, g_dl, g_th = (np.flipud(a) for a in d.get_thomsen_gradients())
    for a in (g_rho, g_vp, g_vs, g_eps, g_dl, g_th):
        assert a.shape == vp.shape and np.isfinite(a).all() and np.abs(a).max() > 0
    # the same by hand: tti.materials + tti.propagate + misfit.l2_half
    dev, h, dt, nt, g, f, pz, px, fw, fsurf = d._setup(model, src, rec)
    prm = [torch.tensor(a.copy(), device=dev, requires_grad=True) for a in (vp, vs, rho, eps, dl, th)]
    mat = tti.materials(*prm, dt, h, free_surface=fsurf)
    vx, vy = tti.propagate(mat, f.to(dev), pz, px, g["sc"], g["sw"], g["rc"], g["rw"], fw, free_surface=fsurf,
                           fd_order=int(d.FD_ORDER))
    tx, ty = (torch.tensor(np.ascontiguousarray(np.transpose(a, (2, 0, 1))), device=dev) for a in (ox, oy))
    hand = misfit.l2_half(vy, ty) + misfit.l2_half(vx, tx)
    hand.backward()
    assert abs(float(hand.detach()) - loss) <= 1e-6 * abs(loss)
    for name, got, p in (("vp", g_vp, prm[0]), ("vs", g_vs, prm[1]), ("rho", g_rho, prm[2]), ("epsilon", g_eps, prm[3]),
                         ("delta", g_dl, prm[4]), ("theta", g_th, prm[5])):
        e = rel_l2(got, p.grad.cpu().numpy())
        print("shim gradient %s vs by hand: rel-L2 %.2e" % (name, e))
        assert e <= 1e-6, name
    # the depth taper reaches all six
    d.SWS_TAPER_GRAD_HOR, d.GRADT1, d.GRADT2, d.GRADT3, d.GRADT4 = 1, 10, 14, 40, 44
    d.grad(model, src, rec)
    tapered = list(d.get_fwi_gradients(["seis"])) + list(d.get_thomsen_gradients())
    assert len(tapered) == 6
    for a in tapered:
        a = np.flipud(a)
        assert not a[:10].any() and not a[44:].any() and np.abs(a[14:40]).max() > 0
    d.SWS_TAPER_GRAD_HOR = 0
    # refusals
    for attr, bad, good in (("INVMAT1", 2, 1), ("EPRECOND", 1, 0), ("SEISMO", 2, 1), ("SEISMO", 4, 1), ("QUELLTYPB", 4, 1),
                            ("acoustic_kernels", "fluid", "elastic"), ("L", 1, 0)):
        setattr(d, attr, bad)
        with pytest.raises(api.MifwiError):
            d.grad(model, src, rec)
        setattr(d, attr, good)
    d.PHYSICS = 5
    with pytest.raises(api.MifwiError, match="4 = P-SV TTI"):
        d.forward(model, src, rec)
    d.PHYSICS = 4
    with pytest.raises(api.MifwiError):
        d.set_thomsen(np.zeros((3, 3)), np.zeros((3, 3)), np.zeros((3, 4)))
    d.set_thomsen(None, None)
    with pytest.raises(api.MifwiError, match="set_thomsen"):
        d.grad(model, src, rec)


# ---- the C entry points -------------------------------------------------------------------------------------------------
def test_c_entry_points_refuse_nulls_bad_ranges_and_born_with_a_force_source():
    from physicsbasedfwi2_amd import _lib, tti, vti
    lib = _lib.load()
    EINVAL = -1
    h = ctypes.c_void_p()
    for bad in (dict(ntap=2), dict(nz=0), dict(nshot=0), dict(source_type=3), dict(fd_order=3), dict(pml_width=-1),
                dict(nz=12, nx=12, pml_width=8)):
        kw = dict(nz=20, nx=24, nt=10, nshot=2, nsrc=1, nrec=3, ntap=1, pml_width=4, free_surface=0, shots_per_group=0,
                  source_type=0, fd_order=4)
        kw.update(bad)
        assert lib.mifwi_tti_plan_create(ctypes.byref(h), 0, ctypes.byref(_lib.TtiDesc(**kw))) == EINVAL, bad
    assert lib.mifwi_tti_plan_create(None, 0, None) == EINVAL
    assert lib.mifwi_tti_plan_layout(None, None) == EINVAL and lib.mifwi_tti_plan_pass_sizes(None, None, None) == EINVAL
    dev = torch.device("cuda:0")
    for st in (0, 1):
        plan = tti.TtiPlan(20, 24, 10, 2, 1, 3, 1, 4, 0, source_type=st)
        other = vti.VtiPlan(20, 24, 10, 2, 1, 3, 1, 4, 0, source_type=st)
        lay = plan.layout
        assert plan.pass_sizes() == (2, lay.ngroups) and plan.cluster_slabs() == 0
        # three strain planes per shot more than the VTI plan's work buffers, and the accumulators of two more planes
        assert lay.snap_step_elems == other.layout.snap_step_elems and lay.state_elems == other.layout.state_elems
        plane = lay.snap_step_elems // (5 * 2)
        assert lay.work_forward_elems == other.layout.work_forward_elems + 3 * 2 * plane
        assert lay.work_backward_elems == other.layout.work_backward_elems + (3 * 2 + 2 * lay.ngroups) * plane
        z = lambda *s: torch.zeros(*s, device=dev)
        mat, pz, px, f = z(8, 20, lay.gp), z(6, 20), z(6, lay.gp), z(10, 2, 1)
        cell, w = torch.zeros(2, 3, 1, dtype=torch.int32, device=dev), z(2, 3, 1)
        scell, sw = torch.zeros(2, 1, 1, dtype=torch.int32, device=dev), z(2, 1, 1)
        rec, snap = z(10, 2, 3), z(10, lay.snap_step_elems)
        work = z(max(lay.work_forward_elems, lay.work_backward_elems))
        P = _lib.ptr
        geo = (P(scell), P(sw), P(cell), P(w))
        fwd = lambda m=P(mat), b=0, e=10, wk=P(work), pl=plan.handle: lib.mifwi_tti_forward(
            pl, m, P(pz), P(px), P(f), *geo, P(rec), P(rec), P(snap), wk, b, e, _lib.ZERO_STATE, None)
        assert fwd(m=None) == EINVAL and fwd(wk=None) == EINVAL and fwd(pl=None) == EINVAL
        assert fwd(b=-1) == EINVAL and fwd(e=11) == EINVAL and fwd(b=5, e=4) == EINVAL
        assert fwd(pl=other.handle) == EINVAL and b"mifwi_tti_plan_create" in lib.mifwi_last_error()
        bwd = lambda s=P(snap), hi=9, lo=0, gx=P(rec): lib.mifwi_tti_backward(
            plan.handle, P(mat), P(pz), P(px), *geo, gx, P(rec), s, 0, P(mat), None, P(work), hi, lo,
            _lib.ZERO_STATE | _lib.FINALIZE, None)
        assert bwd(s=None) == EINVAL and bwd(gx=None) == EINVAL and bwd(hi=10) == EINVAL and bwd(lo=-1) == EINVAL
        born = lambda dm=P(mat), s=P(snap), b=0, e=10: lib.mifwi_tti_born(
            plan.handle, P(mat), dm, P(pz), P(px), None, *geo, s, 0, P(rec), P(rec), P(work), b, e, _lib.ZERO_STATE, None)
        assert born(dm=None) == EINVAL and born(s=None) == EINVAL and born(e=11) == EINVAL
        if st == 1:
            assert born() == EINVAL and b"point-force" in lib.mifwi_last_error()
            assert fwd() == 0 and bwd() == 0                          # a force source is refused by Born alone
        else:
            assert fwd() == 0 and bwd() == 0 and born() == 0          # the valid calls pass
        torch.cuda.synchronize()
        plan.close()
        other.close()
