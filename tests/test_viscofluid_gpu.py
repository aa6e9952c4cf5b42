"""HIP viscoacoustic fluid propagator (viscofluid.propagate / born / gauss_newton_product, mifwi_viscofluid_*) against the
float64 reference of tests/viscofluid_reference.py and against its two exact anchors: the lossless fluid kernels (plane 3
zero) and the viscoelastic P-SV kernels (Vs = 0).

Cases: the four shapes of tests/test_fluid_gpu.py (the three forward tile widths, nx % 4 = 2, 1, 0, two or three adjoint tile
rows) and its four-tap case, 3 shots in groups of 1 and 2 (ragged), 150 steps, a 6-node layer, orders 2 and 4, free surface
0 / 1, explosive / fx / fz; sources on rows >= 1, receivers on rows 15 | 16 where adjoint tiles meet and on row 0 under a
free surface; the Q model of tests/viscofluid_cases.py.  Bounds are the project's: psv_media.TOL_TRACE = 2e-6 for traces
and Born against the reference, TOL_SUM = 2e-5 for sums taken in another order, 1e-6 under a free surface against the
P-SV route."""
import ctypes

import numpy as np
import pytest
import torch

import viscofluid_cases as VC
from cases import FLUID_KINDS as KINDS, rel_l2
from psv_media import PER_STEP, TOL_SUM, TOL_TRACE, check_struct_layouts, close, dot, setenv
from viscofluid_cases import F_REF, F_RELAX, SHAPES, dev, host

pytestmark = pytest.mark.gpu
COMBOS = [(order, fs, st) for order in (2, 4) for fs in (0, 1) for st in (0, 1, 2)]
EINVAL = -1


def _parity(key, st, order, gs, **kw):
    """Traces within TOL_TRACE and the four gradient planes and grad_f within max(TOL_SUM, 4 E_iso) of the float64
    reference; E_iso: today's fluid.propagate against the same reference at qp = inf on the same case, first held to its
    own bound.  Row 0 of planes 0 and 3 is left out under a free surface.  Returns what the run returned."""
    c = VC.case(key)
    iso, ref = VC.ref(key, st, order, "matlim"), VC.ref(key, st, order, "mat4")
    r0 = 1 if c["fs"] else 0
    cut = lambda k, a: a[r0:] if k in ("K", "R") else a
    etr, eg, egf = VC.run(c, c["matlim"][:3], st, order, iso["g"], lossless=True, gs=gs, **kw)
    e_tr = rel_l2(host(etr), iso["rec"])
    e_iso = {k: rel_l2(cut(k, a), cut(k, b)) for k, a, b in zip(("K", "bx", "bz"), eg, iso["planes"][:3])}
    e_iso["f"] = rel_l2(egf, iso["f"])
    print("E_iso %s st %d order %d: traces %.2e, gradients %s" % (key, st, order, e_tr, {k: "%.2e" % v for k, v in e_iso.items()}))
    assert e_tr <= TOL_TRACE, "the lossless kernels miss the trace bound on this case: not a case for this test"
    moved = VC.moved_from_the_limit(key, st, order)
    print("reference vs its qp = inf traces, live shots: %s" % ["%.2e" % v for v in moved])
    assert max(moved) > 0.01                                          # attenuating for real
    tr, vg, vgf = VC.run(c, c["mat4"], st, order, ref["g"], gs=gs, **kw)
    got = host(tr)
    assert all(np.abs(a).max() > 0 for a in ref["rec"]) and all(np.abs(a).max() > 0 for a in got)
    err = rel_l2(got, ref["rec"])
    err_v, err_p = rel_l2(got[:2], ref["rec"][:2]), rel_l2(got[2], ref["rec"][2])
    print("traces vs reference: rel-L2 %.2e (vx, vz %.2e, p %.2e)" % (err, err_v, err_p))
    assert err <= TOL_TRACE and err_v <= TOL_TRACE and err_p <= TOL_TRACE
    for k, a, b in list(zip(VC.PLANES, vg, ref["planes"])) + [("f", vgf, ref["f"])]:
        a, b = cut(k, a), cut(k, b)
        e, tol = rel_l2(a, b), max(TOL_SUM, 4 * e_iso[VC.ISO_OF[k]])
        print("gradient %-2s rel-L2 %.2e (bound %.2e)" % (k, e, tol))
        assert np.abs(b).max() > 0 and np.abs(a).max() > 0, k
        assert e <= tol, (k, e, tol)
    if c["fs"]:
        assert np.isfinite(vg).all()
    return tr, vg, vgf


# ---- 1: parity with the reference -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(SHAPES), ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("order,fs,st", COMBOS)
def test_parity_with_the_reference(shape, order, fs, st):
    """Shot groups of 1 and 2 alternate over the combinations (3 shots: 2 + 1 is ragged)."""
    from physicsbasedfwi2_amd import viscofluid
    nz, nx = shape
    a, b = VC.case((nz, nx, fs))["relax"]
    pl = viscofluid.ViscofluidPlan(nz, nx, 150, 3, 1, 13, 1, 6, 0, a, b)
    assert pl.cluster_slabs(False) == 0 and pl.cluster_slabs(True) == 0
    pl.close()
    _parity((nz, nx, fs), st, order, 1 + (COMBOS.index((order, fs, st)) + nx) % 2)


@pytest.mark.parametrize("fs,st,gs", [(0, 0, 0), (0, 1, 2), (1, 2, 1)])
def test_parity_four_taps(fs, st, gs):
    _parity(("taps4", fs), st, 4, gs)


# ---- 2: the lossless limit ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,order,fs,st", [((37, 70), 4, 0, 0), ((37, 133), 2, 1, 1), ((44, 120), 4, 1, 0), ((23, 240), 2, 0, 2),
                                               ((23, 240), 4, 1, 2)], ids=str)
def test_zero_memory_plane_is_the_fluid_propagator(shape, order, fs, st):
    """mat[3] = 0 on the UNRELAXED planes of the case: fluid.propagate's three traces bit for bit, its three gradient planes
    and grad_f within TOL_SUM; the gradient of plane 3 is finite (and not zero: the derivative with respect to R at R = 0)."""
    key = shape + (fs,)
    c = VC.case(key)
    g = VC.ref(key, st, order, "mat4")["g"]
    m = np.array(c["mat4"])
    m[3] = 0.0
    ftr, fg, fgf = VC.run(c, m[:3], st, order, g, lossless=True, gs=2)
    vtr, vg, vgf = VC.run(c, m, st, order, g, gs=2)
    for name, a, b in zip(("rec_vx", "rec_vz", "rec_p"), vtr, ftr):
        assert b.abs().max() > 0 and torch.equal(a, b), name
    errs = {k: rel_l2(vg[i], fg[i]) for i, k in enumerate(VC.PLANES[:3])}
    errs["f"] = rel_l2(vgf, fgf)
    print("viscofluid(R = 0) vs fluid gradients rel-L2", {k: "%.2e" % v for k, v in errs.items()})
    for k, v in errs.items():
        assert v <= TOL_SUM, (k, v)
    assert np.abs(fg).max() > 0 and np.isfinite(vg[3]).all() and np.abs(vg[3]).max() > 0


# ---- 3: the Vs = 0 limit of the viscoelastic kernels --------------------------------------------------------------------------
@pytest.mark.parametrize("shape,order,fs,st", [((37, 70), 4, 0, 0), ((37, 133), 2, 0, 1), ((44, 120), 4, 0, 2), ((23, 240), 2, 0, 0),
                                               ((37, 70), 4, 1, 0), ((23, 240), 4, 1, 2)], ids=str)
def test_against_the_viscoelastic_route_with_vs_zero(monkeypatch, shape, order, fs, st):
    """visco.propagate on visco.materials(vp, 0, rho, qp, inf, ...), one launch per half step: rec_vx, rec_vz bit for bit
    without a free surface, <= 1e-6 with one (the P-SV route's effective row 0 is zero only up to rounding).  Both routes get
    the planes of one float64 evaluation rounded to f32.  The gradient differences are printed, not bounded: the P-SV
    route's sxx_bar and szz_bar drift apart in f32 while only their sum is the adjoint pressure."""
    from physicsbasedfwi2_amd import visco
    setenv(monkeypatch, PER_STEP)
    key = shape + (fs,)
    c = VC.case(key)
    t = lambda a: torch.tensor(VC.f32(a), dtype=torch.float64)
    vp = t(c["vp"])
    m8 = VC.f32(visco.materials(vp, torch.zeros_like(vp), t(c["rho"]), t(c["qp"]), torch.full_like(vp, float("inf")), F_REF,
                                F_RELAX, c["dt"], c["h"], free_surface=bool(fs)).numpy())
    r0 = 1 if fs else 0
    assert np.array_equal(m8[0][r0:], c["mat4"][0][r0:]) and np.array_equal(m8[6][r0:], c["mat4"][3][r0:])
    assert np.array_equal(m8[3:5], c["mat4"][1:3]) and np.array_equal(m8[0][r0:], m8[1][r0:])
    g = VC.ref(key, st, order, "mat4")["g"]
    vtr, vg, vgf = VC.run(c, c["mat4"], st, order, g[:2] + [np.zeros_like(g[2])], gs=2)
    mat = dev(m8).requires_grad_(True)
    f = dev(c["f"]).requires_grad_(True)
    pvx, pvz = visco.propagate(*VC.args(c, mat, f), F_RELAX, c["dt"], shots_per_group=2, free_surface=bool(fs),
                               source_type=KINDS[st], fd_order=order)
    torch.autograd.backward([pvx, pvz], [dev(a) for a in g[:2]])
    pg = mat.grad.double().cpu().numpy()
    assert pvx.abs().max() > 0 and pvz.abs().max() > 0
    e = rel_l2(host(vtr[:2]), host([pvx.detach(), pvz.detach()]))
    print("viscofluid vs visco(Vs = 0) traces rel-L2 %.2e" % e)
    if fs:
        assert e <= 1e-6
    else:
        assert torch.equal(vtr[0], pvx.detach()) and torch.equal(vtr[1], pvz.detach())
    diffs = dict(K=rel_l2(vg[0][r0:], (pg[0] + pg[1])[r0:]), bx=rel_l2(vg[1], pg[3]), bz=rel_l2(vg[2], pg[4]),
                 R=rel_l2(vg[3][r0:], (pg[5] + pg[6])[r0:]), f=rel_l2(vgf, f.grad.double().cpu().numpy()))
    print("viscofluid vs visco(Vs = 0) gradients rel-L2 (not bounded)", {k: "%.2e" % v for k, v in diffs.items()})


# ---- 4: Born modelling and Gauss-Newton products --------------------------------------------------------------------------------
def _born(c, st, order=4, dmat=None, df=None, **kw):
    from physicsbasedfwi2_amd import viscofluid
    a = VC.args(c, dev(c["mat4"]))
    return viscofluid.born(a[0], dev(c["dmat"]) if dmat is None else dmat, *a[1:], F_RELAX, c["dt"], df=df,
                           free_surface=bool(c["fs"]), source_type=KINDS[st], record_pressure=True, fd_order=order, **kw)


@pytest.mark.parametrize("shape,order,fs,st", [((37, 70), 4, 0, 0), ((37, 70), 2, 1, 1), ((37, 133), 2, 0, 2), ((37, 133), 4, 1, 0),
                                               ((44, 120), 4, 0, 1), ((44, 120), 2, 1, 2), ((23, 240), 2, 0, 0), ((23, 240), 4, 1, 1),
                                               ((23, 240), 4, 0, 2)], ids=str)
def test_born_is_the_directional_derivative_of_the_reference(shape, order, fs, st):
    """J (dmat, df) against the central difference of the float64 reference (eps = 1e-5), (dvx, dvz) and drec_p, every tile
    width with every source type."""
    key = shape + (fs,)
    c = VC.case(key)
    want = VC.ref_jvp(key, st, order)
    out = _born(c, st, order, df=dev(c["df"]))
    assert len(out) == 6
    got = host(out[3:])
    ev, ep = rel_l2(got[:2], want[:2]), rel_l2(got[2], want[2])
    print("born vs central difference of the reference %s order %d st %d: rel-L2 v %.3e p %.3e" % (key, order, st, ev, ep))
    assert np.abs(want[:2]).max() > 0 and np.abs(want[2]).max() > 0 and np.abs(got[2]).max() > 0
    assert ev <= TOL_TRACE and ep <= TOL_TRACE
    bg = VC.run(c, c["mat4"], st, order)
    for a, b in zip(out[:3], bg):
        assert torch.equal(a, b)                               # the background traces are propagate's


@pytest.mark.parametrize("shape,fs,st", [((37, 133), 0, 0), ((23, 240), 1, 1), ((44, 120), 1, 2)], ids=str)
def test_born_is_the_transpose_partner_of_the_gradients_and_the_product_is_the_composition(shape, fs, st):
    """<J (dm, df), g> = <dm, mat.grad> + <df, f.grad> of propagate + backward(g) within 2e-5, the fluid Born test's bound
    for sums taken in another order; hv of gauss_newton_product is propagate + backward(drec) bit for bit."""
    from physicsbasedfwi2_amd import viscofluid
    c = VC.case(shape + (fs,))
    dm, df = dev(c["dmat"]), dev(c["df"])
    drec = _born(c, st, df=df)[3:]
    g = [torch.sign(a) + 0.5 for a in drec]
    mat, f = dev(c["mat4"]).requires_grad_(True), dev(c["f"]).requires_grad_(True)
    run = lambda: viscofluid.propagate(*VC.args(c, mat, f), F_RELAX, c["dt"], free_surface=bool(fs), source_type=KINDS[st],
                                       record_pressure=True)
    torch.autograd.backward(list(run()), g)
    close(sum(dot(a, b) for a, b in zip(drec, g)), dot(dm, mat.grad) + dot(df, f.grad), 2e-5, "<J d, g> vs <d, J^T g>")
    assert float(mat.grad[3].abs().max()) > 0
    a = VC.args(c, dev(c["mat4"]))
    hv, *drec2 = viscofluid.gauss_newton_product(a[0], dm, *a[1:], F_RELAX, c["dt"], df=df, free_surface=bool(fs),
                                                 source_type=KINDS[st], record_pressure=True)
    for x, y in zip(drec, drec2):
        assert torch.equal(x, y)
    mat.grad = None
    torch.autograd.backward(list(run()), list(drec))
    assert hv.shape == mat.shape and float(hv.abs().max()) > 0 and torch.equal(hv, mat.grad)


def test_born_in_shot_chunks_gives_the_bits_of_the_whole_run():
    from physicsbasedfwi2_amd import viscofluid
    c = VC.case((37, 133, 0))
    a, b = c["relax"]
    pl = viscofluid.ViscofluidPlan(37, 133, 150, 1, 1, 13, 1, c["fw"], 0, a, b)
    one_shot = 4 * 150 * pl.layout.snap_step_elems
    pl.close()
    whole = _born(c, 2)
    assert len(whole) == 6 and all(t.abs().max() > 0 for t in whole)
    chunked = _born(c, 2, snapshot_budget=int(1.5 * one_shot))         # holds one shot's snapshots, not two
    for x, y in zip(whole, chunked):
        assert torch.equal(x, y)
    with pytest.raises(viscofluid.MifwiError, match="checkpoints"):
        _born(c, 2, snapshot_budget=one_shot // 2)


# ---- 5: the forms of the driver -----------------------------------------------------------------------------------------------
def _bits(key, st, gs, **kw):
    c = VC.case(key)
    g = VC.ref(key, st, 4, "mat4")["g"]
    tr, gm, gf = VC.run(c, c["mat4"], st, 4, g, gs=gs, **kw)
    return [t.cpu().numpy() for t in tr] + [gm, gf]


@pytest.mark.parametrize("fs,st", [(0, 0), (1, 1), (0, 2)])
def test_one_shot_passes_equal_the_unsplit_run(monkeypatch, fs, st):
    """MIFWI_FL_PASS_SHOTS = MIFWI_FL_PASS_GROUPS = 1: the forward sweeps the time range shot by shot, the adjoint group by
    group (3 shots in groups of 2), with g_vx, g_vz and g_p: the bits of the unsplit run."""
    from physicsbasedfwi2_amd import viscofluid
    key = (37, 133, fs)
    a, b = VC.case(key)["relax"]
    runs = []
    for split in (False, True):
        for name in ("MIFWI_FL_PASS_SHOTS", "MIFWI_FL_PASS_GROUPS"):
            monkeypatch.setenv(name, "1") if split else monkeypatch.delenv(name, raising=False)
        pl = viscofluid.ViscofluidPlan(37, 133, 150, 3, 1, 13, 1, 6, 0, a, b, 2, fs, st, 4)
        assert pl.layout.ngroups == 2 and pl.pass_sizes() == ((1, 1) if split else (3, 2))
        pl.close()
        runs.append(_bits(key, st, 2))
    assert all(np.abs(x).max() > 0 for x in runs[0])
    for name, x, y in zip(("rec_vx", "rec_vz", "rec_p", "grad_mat", "grad_f"), runs[0], runs[1]):
        assert np.array_equal(x, y), name


def test_checkpoints_carry_the_memory_variable_and_calls_repeat():
    """Three time-checkpoint segments: the trace bits of the resident run, gradients within TOL_SUM (the value is printed);
    state_elems holds four fields per shot; a second identical call returns the bits of the first."""
    from physicsbasedfwi2_amd import fluid, viscofluid
    from physicsbasedfwi2_amd._driver import checkpoint_schedule, segment_length
    key = (37, 70, 1)
    c = VC.case(key)
    a, b = c["relax"]
    pl = viscofluid.ViscofluidPlan(37, 70, 150, 3, 1, 13, 1, 6, 0, a, b, 2, 1, 1, 4)
    fl = fluid.FluidPlan(37, 70, 150, 3, 1, 13, 1, 6, 0, 2, 1, 1, 4)
    lay, flay = pl.layout, fl.layout
    field = (37 + 4) * lay.pitch * 3
    assert lay.state_elems - flay.state_elems == field and lay.state_elems >= 4 * field
    assert lay.snap_step_elems == flay.snap_step_elems and lay.work_backward_elems - flay.work_backward_elems >= field
    sb = 4 * lay.snap_step_elems
    pl.close(), fl.close()
    seg = segment_length(2 * 50 * sb, torch.device(VC.DEV), sb, 150)
    assert seg == 50 and len(checkpoint_schedule(150, seg, "elastic")[0]) == 3
    first, again, cut = _bits(key, 1, 2), _bits(key, 1, 2), _bits(key, 1, 2, snapshot_budget=2 * 50 * sb)
    assert all(np.abs(x).max() > 0 for x in first)
    for x, y in zip(first, again):
        assert np.array_equal(x, y), "repeated call"
    for x, y in zip(first[:3], cut[:3]):
        assert np.array_equal(x, y), "three checkpoint segments: traces"
    e = max(rel_l2(cut[3][k], first[3][k]) for k in range(4)), rel_l2(cut[4], first[4])
    print("three checkpoint segments vs resident: grad_mat rel-L2 %.2e (worst plane), grad_f %.2e" % e)
    assert max(e) <= TOL_SUM


# ---- 6: the C entry points ----------------------------------------------------------------------------------------------------
def test_c_entry_points_refuse_nulls_bad_ranges_and_the_other_family(tmp_path):
    from physicsbasedfwi2_amd import _lib, fluid, viscofluid
    lib = _lib.load()
    check_struct_layouts({"mifwi_viscofluid_desc": _lib.ViscofluidDesc, "mifwi_viscofluid_layout": _lib.ViscofluidLayout,
                          "mifwi_fluid_desc": _lib.FluidDesc, "mifwi_fluid_layout": _lib.FluidLayout}, tmp_path)
    h = ctypes.c_void_p()
    for bad in (dict(ntap=2), dict(nz=0), dict(nshot=0), dict(source_type=3), dict(fd_order=3), dict(pml_width=-1),
                dict(nz=12, nx=12, pml_width=8), dict(free_surface=1, nz=2), dict(relax_a=0.0), dict(relax_a=1.0),
                dict(relax_b=0.0), dict(relax_b=2.0), dict(relax_a=float("nan"))):
        kw = dict(nz=20, nx=24, nt=10, nshot=2, nsrc=1, nrec=3, ntap=1, pml_width=4, free_surface=0, shots_per_group=0,
                  source_type=0, fd_order=4, relax_a=0.9, relax_b=0.1)
        kw.update(bad)
        assert lib.mifwi_viscofluid_plan_create(ctypes.byref(h), 0, ctypes.byref(_lib.ViscofluidDesc(**kw))) == EINVAL, bad
    assert lib.mifwi_viscofluid_plan_create(None, 0, None) == EINVAL
    assert lib.mifwi_viscofluid_plan_layout(None, None) == EINVAL and lib.mifwi_viscofluid_plan_pass_sizes(None, None, None) == EINVAL
    d = torch.device(VC.DEV)
    P, N = _lib.ptr, None
    for st in (0, 1):
        plan = viscofluid.ViscofluidPlan(20, 24, 10, 2, 1, 3, 1, 4, 0, 0.9, 0.1, source_type=st)
        lay = plan.layout
        assert plan.pass_sizes() == (2, lay.ngroups) and plan.cluster_slabs() == 0
        z = lambda *s: torch.zeros(*s, device=d)
        mat, pz, px, f = z(4, 20, lay.gp), z(6, 20), z(6, lay.gp), z(10, 2, 1)
        cell, w = torch.zeros(2, 3, 1, dtype=torch.int32, device=d), z(2, 3, 1)
        scell, sw = torch.zeros(2, 1, 1, dtype=torch.int32, device=d), z(2, 1, 1)
        rec, snap = z(10, 2, 3), z(10, lay.snap_step_elems)
        work = z(max(lay.work_forward_elems, lay.work_backward_elems))
        geo = (P(scell), P(sw), P(cell), P(w))
        fwd = lambda m=P(mat), b=0, e=10, wk=P(work), rvz=P(rec): lib.mifwi_viscofluid_forward(
            plan.handle, m, P(pz), P(px), P(f), *geo, P(rec), rvz, P(rec), P(snap), wk, b, e, _lib.ZERO_STATE, None)
        assert fwd(m=None) == EINVAL and fwd(wk=None) == EINVAL and fwd(rvz=None) == EINVAL
        assert fwd(b=-1) == EINVAL and fwd(e=11) == EINVAL and fwd(b=5, e=4) == EINVAL
        assert lib.mifwi_viscofluid_forward(None, P(mat), P(pz), P(px), P(f), *geo, P(rec), P(rec), P(rec), P(snap), P(work), 0,
                                            10, 1, None) == EINVAL
        bwd = lambda s=P(snap), hi=9, lo=0, first=0, gm=P(mat): lib.mifwi_viscofluid_backward(
            plan.handle, P(mat), P(pz), P(px), *geo, P(rec), P(rec), P(rec), s, first, gm, None, P(work), hi, lo,
            _lib.ZERO_STATE | _lib.FINALIZE, None)
        assert bwd(s=None) == EINVAL and bwd(hi=10) == EINVAL and bwd(lo=-1) == EINVAL and bwd(first=1) == EINVAL
        assert bwd(gm=None) == EINVAL                                        # finalize without grad_mat
        born = lambda dm=P(mat), s=P(snap), b=0, e=10, first=0: lib.mifwi_viscofluid_born(
            plan.handle, P(mat), dm, P(pz), P(px), None, *geo, s, first, P(rec), P(rec), P(rec), P(work), b, e, _lib.ZERO_STATE,
            None)
        assert born(dm=None) == EINVAL and born(s=None) == EINVAL and born(e=11) == EINVAL
        assert born(first=-1) == EINVAL and born(b=2, first=3) == EINVAL
        assert fwd() == 0 and bwd() == 0 and born() == 0                     # the valid calls pass, force sources included
        torch.cuda.synchronize()
        # the handle types are kept apart: refused before anything else is read (all other arguments null)
        for call in (lambda: lib.mifwi_fluid_forward(plan.handle, *[N] * 13, 0, 10, 0, N),
                     lambda: lib.mifwi_fluid_backward(plan.handle, *[N] * 11, 0, N, N, N, 9, 0, 0, N),
                     lambda: lib.mifwi_fluid_born(plan.handle, *[N] * 10, 0, N, N, N, N, 0, 10, 0, N),
                     lambda: lib.mifwi_fluid_snapshot_moments(plan.handle, N, 0, 0, 10, 1, N, N, 0, N)):
            assert call() == EINVAL and b"not created by mifwi_fluid_plan_create" in lib.mifwi_last_error()
        plan.close()
    other = fluid.FluidPlan(20, 24, 10, 2, 1, 3, 1, 4, 0)
    for call in (lambda: lib.mifwi_viscofluid_forward(other.handle, *[N] * 13, 0, 10, 0, N),
                 lambda: lib.mifwi_viscofluid_backward(other.handle, *[N] * 11, 0, N, N, N, 9, 0, 0, N),
                 lambda: lib.mifwi_viscofluid_born(other.handle, *[N] * 10, 0, N, N, N, N, 0, 10, 0, N)):
        assert call() == EINVAL and b"not created by mifwi_viscofluid_plan_create" in lib.mifwi_last_error()
    other.close()


def test_python_refusals():
    from physicsbasedfwi2_amd import fluid, viscofluid
    c = VC.case((37, 70, 0))
    a = VC.args(c, dev(c["mat4"]))
    with pytest.raises(viscofluid.MifwiError, match="pseudo_hessian"):
        viscofluid.propagate(*a, F_RELAX, c["dt"], pseudo_hessian=fluid.PseudoHessian())
    with pytest.raises(viscofluid.MifwiError, match=r"\[4, nz, nx\]"):
        viscofluid.propagate(dev(c["mat4"][:3]), *a[1:], F_RELAX, c["dt"])
    with pytest.raises(viscofluid.MifwiError, match="inside"):
        viscofluid.propagate(*a, 400.0, c["dt"])
    with pytest.raises(viscofluid.MifwiError, match="dmat"):
        viscofluid.born(a[0], dev(c["dmat"][:3]), *a[1:], F_RELAX, c["dt"])


# ---- 7: the pyapi_denise switch -------------------------------------------------------------------------------------------------
def _denise(tmp_path, L, free_surf=1):
    import physicsbasedfwi2_amd.compat.pyapi_denise as api
    rng = np.random.default_rng(3)
    nz, nx, dx = 48, 70, 20.0
    vp = (1800 + 1200 * rng.random((nz, nx))).astype(np.float32)
    rho = (1900 + 300 * rng.random((nz, nx))).astype(np.float32)
    d = api.Denise("/nonexistent", verbose=0)
    d.save_folder = str(tmp_path)
    d.PHYSICS, d.ITERMAX, d.L, d.FL1, d.acoustic_kernels = 2, 1, L, 8.0, "fluid"
    d.TIME, d.DT, d.FREE_SURF, d.FW, d.FPML, d.DAMPING = 0.3, 0.0015, free_surf, 8, 5.0, 1500.0
    d.QUELLTYP, d.SEISMO, d.QUELLTYPB = 2, 4, 1
    xsrc = np.array([400.0, 1000.0])
    src = api.Sources(xsrc, 40.0 * xsrc / xsrc, 8.0)
    xrec = np.arange(300.0, 1100.0 + dx, 40.0)
    rec = api.Receivers(xrec, 460.0 * (xrec / xrec))
    z, x = np.meshgrid(np.arange(nz) / nz, np.arange(nx) / nx, indexing="ij")
    qp = (60 + 35 * np.sin(5 * z + 3 * x)).astype(np.float32)
    return api, d, (vp, rho, qp), dx, src, rec


def test_shim_by_hand_lossless_limit_q_gradient_and_refusals(tmp_path, monkeypatch):
    """PHYSICS = 2, acoustic_kernels = "fluid", L = 1 (force x, velocities and pressure recorded, a free surface): loss and
    gradients are the by-hand composition viscofluid.materials -> propagate -> misfit.l2_half -> backward bit for bit; qp =
    inf gives the L = 0 fluid seismograms bit for bit; get_attenuation_gradients() returns the by-hand Qp gradient and zeros
    for Qs; the refusals come before the device is touched."""
    from physicsbasedfwi2_amd import fluid, misfit, viscofluid
    monkeypatch.chdir(tmp_path)
    api, d, (vp, rho, qp), dx, src, rec = _denise(tmp_path, 1)
    zero = np.zeros_like(vp)
    model = api.Model(np.flipud(vp), np.flipud(zero), np.flipud(rho), dx)

    def current_device():
        raise AssertionError("the device was touched")
    with monkeypatch.context() as m:
        m.setattr(torch.cuda, "current_device", current_device)
        d.set_observed(np.zeros((2, 200, 21)), np.zeros((2, 200, 21)))
        with pytest.raises(api.MifwiError, match="set_attenuation"):
            d.forward(model, src, rec)                                              # missing Q arrays
        with pytest.raises(api.MifwiError, match="set_attenuation"):
            d.grad(model, src, rec)
        with pytest.raises(api.MifwiError):
            d.set_attenuation(np.flipud(qp), None)
        d.set_attenuation(np.flipud(qp), np.flipud(qp))
        for attr, bad, good, msg in (("EPRECOND", 1, 0, "EPRECOND"), ("acoustic_kernels", "elastic", "fluid", "L=1")):
            setattr(d, attr, bad)
            with pytest.raises(api.MifwiError, match=msg):
                d.forward(model, src, rec)
            with pytest.raises(api.MifwiError, match=msg):
                d.grad(model, src, rec)
            setattr(d, attr, good)
        with pytest.raises(api.MifwiError):
            d.get_attenuation_gradients()
    # forward against the by-hand composition
    sx, sy = d.forward(model, src, rec)
    sp = np.stack(d.get_shots(keys=["_p"]))
    dev_, h, dt, nt, g, f, pz, px, fw, fsurf = d._setup(model, src, rec)
    f_ref = 8.0                                                  # F_REF = None: the first source's centre frequency

    def hand(vp_t, rho_t, qp_t):
        mat = viscofluid.materials(vp_t, rho_t, qp_t, f_ref, d.FL1, dt, h, free_surface=fsurf)
        ff = fluid.force_amplitude(f.to(dev_), mat, g["sc"], g["sw"], h, "fx")
        return viscofluid.propagate(mat, ff, pz, px, g["sc"], g["sw"], g["rc"], g["rw"], fw, d.FL1, dt, free_surface=fsurf,
                                    source_type="fx", record_pressure=True, fd_order=int(d.FD_ORDER))
    tens = lambda a, **kw: torch.tensor(a.copy(), device=dev_, **kw)
    with torch.no_grad():
        hx, hy, hp = hand(tens(vp), tens(rho), tens(qp))
    perm = lambda t: t.permute(1, 2, 0).cpu().numpy()
    assert np.abs(sx).max() > 0 and np.abs(sp).max() > 0
    assert np.array_equal(sx, perm(hx)) and np.array_equal(sy, perm(hy)) and np.array_equal(sp, -perm(hp))
    # the stability limit is taken at the unrelaxed velocity
    from physicsbasedfwi2_amd import profiles
    vmax = viscofluid.max_velocity(vp, qp, f_ref, d.FL1)
    assert vmax > float(vp.max())
    d.DT = 0.5 * (profiles.elastic_cfl_limit(h, vmax, int(d.FD_ORDER)) + profiles.elastic_cfl_limit(h, float(vp.max()), int(d.FD_ORDER)))
    with pytest.raises(api.MifwiError, match="stability"):
        d.forward(model, src, rec)
    d.DT = 0.0015
    # qp = inf: the L = 0 fluid seismograms, bit for bit
    inf = np.full_like(vp, np.inf)
    d.set_attenuation(inf, inf)
    ix, iy = d.forward(model, src, rec)
    ip = np.stack(d.get_shots(keys=["_p"]))
    _, d0, _, _, _, _ = _denise(tmp_path, 0)
    ex, ey = d0.forward(model, src, rec)
    ep = np.stack(d0.get_shots(keys=["_p"]))
    assert np.abs(ex).max() > 0 and np.array_equal(ix, ex) and np.array_equal(iy, ey) and np.array_equal(ip, ep)
    moved = rel_l2(np.stack([sx, sy]), np.stack([ex, ey]))
    print("attenuating vs L = 0 seismograms: rel-L2 %.2e" % moved)
    assert moved > 0.01
    # loss and gradients against autograd through the by-hand composition, Q held fixed in the change of variables
    d.set_attenuation(np.flipud(qp * 1.2), np.flipud(qp))
    ox, oy = d.forward(api.Model(np.flipud(vp * 1.03), np.flipud(zero), np.flipud(rho), dx), src, rec)
    d.set_observed(np.transpose(ox, (0, 2, 1)), np.transpose(oy, (0, 2, 1)))
    d.set_attenuation(np.flipud(qp), np.flipud(qp))
    prm = [tens(a, requires_grad=True) for a in (vp, rho, qp)]
    vx, vy, _ = hand(*prm)
    tx, ty = (torch.tensor(np.ascontiguousarray(np.transpose(a, (2, 0, 1))), device=dev_) for a in (ox, oy))
    by_hand = misfit.l2_half(vy, ty) + misfit.l2_half(vx, tx)
    by_hand.backward()
    loss = d.grad(model, src, rec)
    assert loss > 0 and loss == float(by_hand.detach())
    g_rho, g_vp, g_vs = (np.flipud(a) for a in d.get_fwi_gradients(["seis"]))
    g_qp, g_qs = (np.flipud(a) for a in d.get_attenuation_gradients())
    for nm, got, want in (("vp", g_vp, prm[0].grad), ("rho", g_rho, prm[1].grad), ("qp", g_qp, prm[2].grad)):
        assert got.shape == vp.shape and np.abs(got).max() > 0, nm
        assert np.array_equal(got, want.cpu().numpy()), nm
    assert not g_vs.any() and not g_qs.any() and g_qs.shape == vp.shape
    with pytest.raises(api.MifwiError):
        d0.get_attenuation_gradients()
