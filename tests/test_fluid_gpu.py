"""HIP fluid (variable-density acoustic) propagator against the CPU oracle of the elastic scheme (fp32) run on
mat5 = [K, K, 0, bx, bz], and against the library's own elastic route.

With Ms == Ls the oracle's two stress updates are one fmaf chain on the same operands, so the seismograms (vx, vz and
p + p = sxx + szz) are required to be the same bits; the adjoint sums sxx_bar + szz_bar in another order, so the
gradients are held to the elastic tests' rel-L2 <= 2e-5 (grad_mat[0] against gL + gM).  Under a free surface row 0 of
both K planes is 0, explosive sources sit on rows >= 1 (on row 0 the two models differ by construction) and so do the
force sources.

The checker has an error of its own in gL + gM: its sxx_bar and szz_bar drift apart while only their sum is the adjoint
pressure, so gL and gM can each be many times their sum and the f32 sum loses those digits (a source in the corner of
the layer, 100 steps: |gL| = 75 |gL + gM|, f32 oracle 3.6e-5 from the f64 oracle).  Every case here is therefore
required to keep the f32 oracle within a quarter of the bound of the f64 oracle before the library is compared with it.
"""
import functools

import numpy as np
import pytest
import torch

from cases import (FLUID_KINDS as KINDS, FLUID_TOL_GRAD as TOL_GRAD, elastic_case, elastic_case_taps4, fluid_backward,
                   fluid_check, fluid_oracle, fluid_planes as _fluid_planes, fluid_run, rel_l2)
from oracle import helpers as H

pytestmark = pytest.mark.gpu
TOL_TRACE = 1e-6
DEV = "cuda:0"
# nz x nx -> lanes per row of the forward tiles by the plan's rule (mifwi::pick_lx on 18, 34, 30 and 60 four-cell groups per
# row): the three widths the family instantiates; nx % 4 = 2, 1, 0; two or three adjoint tile rows, two to four tile columns
SHAPES = {(37, 70): 16, (37, 133): 16, (44, 120): 32, (23, 240): 64}


@functools.lru_cache(maxsize=None)
def _case(nz, nx, fs, nt=150, seed=7):
    """Three shots (a ragged shot group), one source each on rows 1 .. 4, receivers on the rows 15 | 16 where the adjoint
    tiles meet (shot 0 under a free surface: on the surface row), the source of shot 0 inside the left layer."""
    c = elastic_case(seed=seed, nz=nz, nx=nx, fw=6, nt=nt, ns=3, nsrc=1, nrec=13, water=0, free_surface=bool(fs))
    sc = c["sc"].copy()
    sc[0, 0, 0] = (sc[0, 0, 0] // nx) * nx + 3     # inside the C-PML on the left
    if fs:
        sc = np.where(sc // nx == 0, sc + nx, sc)      # off the surface row
        assert (sc // nx >= 1).all()
    c["sc"] = sc.astype(np.int32)
    rx = np.linspace(2, nx - 3, 13).astype(int)
    rows = [0 if fs else 15, 16, 15]
    c["rc"] = np.stack([(r * nx + rx) for r in rows])[:, :, None].astype(np.int32)
    c["rw"] = np.ones(c["rc"].shape)
    return _fluid_planes(c, fs)


@functools.lru_cache(maxsize=None)
def _oracle_run(key, st, order):
    """The oracle's traces, the adjoint inputs, its gradients (shared by the tests of one case, never modified) and the
    distance of its gL + gM from the f64 oracle's."""
    return fluid_oracle(_CASES[key](), st, order)


_CASES = {}
for (_nz, _nx) in SHAPES:
    for _fs in (0, 1):
        _CASES[(_nz, _nx, _fs)] = functools.partial(_case, _nz, _nx, _fs)
_CASES[("taps4", 0)] = lambda: _taps4(False)
_CASES[("taps4", 1)] = lambda: _taps4(True)


@functools.lru_cache(maxsize=None)
def _taps4(fs):
    """Bilinear four-tap sources and receivers, at most two receiver taps of a shot per cell; Vs dropped.  Under a free
    surface the sources go one row down (source 1 of shot 0 would touch row 0)."""
    kw = dict(ns=3, water=0)
    c = elastic_case_taps4("U", 21, free_surface=fs, **kw)
    if fs:
        nz, nx = c["vp"].shape
        src = c["src_zx"].copy()
        src[..., 0] = np.maximum(src[..., 0], 1.3)
        c["sc"], c["sw"] = H.bilinear_taps(src * c["h"], (c["h"], c["h"]), 0, (nz, nx))
        assert (c["sc"] // nx >= 1).all()
    return _fluid_planes(c, fs)


def _run_hip(c, st, order, gs=0, budget=None):
    return fluid_run(c, st, order, gs, budget)


def _backward(out, g):
    fluid_backward(out, g)


def _check_parity(key, st, order, gs):
    fluid_check(_CASES[key](), _oracle_run(key, st, order), st, order, gs)


COMBOS = [(order, fs, st) for order in (2, 4) for fs in (0, 1) for st in (0, 1, 2)]


@pytest.mark.parametrize("shape", list(SHAPES), ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("order,fs,st", COMBOS)
def test_parity_with_the_oracle(shape, order, fs, st):
    """Bitwise traces, 2e-5 gradients; shot groups of 1 and 2 alternate over the combinations (3 shots: 2 + 1 is ragged)."""
    from physicsbasedfwi2_amd import fluid
    nz, nx = shape
    pl = fluid.FluidPlan(nz, nx, 150, 3, 1, 13, 1, 6, 0)
    assert pl.cluster_slabs(False) == 0 and pl.cluster_slabs(True) == 0
    pl.close()
    _check_parity((nz, nx, fs), st, order, 1 + (COMBOS.index((order, fs, st)) + nx) % 2)


@pytest.mark.parametrize("fs,st", [(0, 0), (1, 1), (0, 2)])
def test_one_shot_passes_equal_the_unsplit_run(monkeypatch, fs, st):
    """The Infinity-Cache passes: MIFWI_FL_PASS_SHOTS = MIFWI_FL_PASS_GROUPS = 1 makes the forward sweep the time range shot
    by shot and the adjoint group by group (3 shots in groups of 2: the last group is ragged), which on these grids the
    plan's own rule never does.  Shots and groups are independent, so traces, grad_mat and grad_f - with g_vx, g_vz and
    g_p - must be the bits of the unsplit run."""
    from physicsbasedfwi2_amd import fluid
    c = _case(37, 133, fs, nt=90, seed=11)
    rng = np.random.default_rng(4)
    runs = []
    for split in (False, True):
        for name in ("MIFWI_FL_PASS_SHOTS", "MIFWI_FL_PASS_GROUPS"):
            monkeypatch.setenv(name, "1") if split else monkeypatch.delenv(name, raising=False)
        pl = fluid.FluidPlan(37, 133, 90, 3, 1, 13, 1, 6, 0, 2, fs, st, 4)
        assert pl.layout.ngroups == 2 and pl.pass_sizes() == ((1, 1) if split else (3, 2))
        pl.close()
        mat, f, out = _run_hip(c, st, 4, gs=2)
        if not runs:
            g = [(rng.standard_normal(tuple(a.shape)) * float(a.detach().abs().max())).astype(np.float32) for a in out]
        _backward(out, g)
        runs.append([a.detach().cpu().numpy() for a in out] + [mat.grad.cpu().numpy(), f.grad.cpu().numpy()])
    assert all(np.abs(a).max() > 0 for a in runs[0])
    for name, a, b in zip(("rec_vx", "rec_vz", "rec_p", "grad_mat", "grad_f"), runs[0], runs[1]):
        assert np.array_equal(a, b), name


@pytest.mark.parametrize("fs,st,gs", [(0, 0, 0), (0, 1, 2), (1, 2, 1)])
def test_parity_four_taps(fs, st, gs):
    _check_parity(("taps4", fs), st, 4, gs)


@pytest.mark.parametrize("fs,st", [(0, 0), (0, 1), (1, 0), (1, 2)])
def test_against_the_elastic_route(fs, st):
    """elastic.propagate on staggered_materials(vp, 0, rho): the same traces (bitwise; within 1e-6 under a free surface,
    where the elastic route's effective row 0 is not exactly 0), the same Vp and rho gradients after the chain rule, and
    no Vs gradient."""
    from physicsbasedfwi2_amd import elastic, fluid
    c = _case(37, 70, fs)
    tens = lambda a, **k: torch.tensor(a, dtype=torch.float32, device=DEV, **k)
    geo = [torch.tensor(c[k]) for k in ("sc", "sw", "rc", "rw")]
    pz, px = torch.tensor(c["pz"]), torch.tensor(c["px"])
    rng = np.random.default_rng(5)
    res = {}
    for route in ("elastic", "fluid"):
        vp, rho = tens(c["vp"], requires_grad=True), tens(c["rho"], requires_grad=True)
        vs = torch.zeros_like(vp, requires_grad=True)
        f = tens(c["f"])
        if route == "elastic":
            mat = elastic.staggered_materials(vp, vs, rho, c["dt"], c["h"], free_surface=bool(fs))
            if st:
                f = elastic.force_amplitude(f, mat, geo[0], geo[1], c["h"], KINDS[st])
            out = elastic.propagate(mat, f, pz, px, *geo, c["fw"], free_surface=bool(fs), source_type=KINDS[st],
                                    record_pressure=True, fd_order=4)
        else:
            mat = fluid.materials(vp, rho, c["dt"], c["h"], free_surface=bool(fs))
            if st:
                f = fluid.force_amplitude(f, mat, geo[0], geo[1], c["h"], KINDS[st])
            out = fluid.propagate(mat, f, pz, px, *geo, c["fw"], free_surface=bool(fs), source_type=KINDS[st],
                                  record_pressure=True, fd_order=4)
        if route == "elastic":
            g = [torch.tensor((rng.standard_normal(tuple(a.shape)) * float(a.detach().abs().max())).astype(np.float32), device=DEV)
                 for a in out]
        torch.autograd.backward(list(out), g)
        res[route] = ([a.detach().cpu().numpy() for a in out], vp.grad.cpu().numpy(), rho.grad.cpu().numpy(),
                      None if vs.grad is None else vs.grad.cpu().numpy())
    (te, gvp_e, grho_e, gvs_e), (tf, gvp_f, grho_f, _) = res["elastic"], res["fluid"]
    for name, a, b in zip(("rec_vx", "rec_vz", "rec_p"), tf, te):
        assert np.abs(b).max() > 0
        print("%s rel-L2 %.2e" % (name, rel_l2(a, b)))
        if fs:
            assert rel_l2(a, b) <= TOL_TRACE, name
        else:
            assert np.array_equal(a, b), name
    print("vp.grad rel-L2 %.2e rho.grad %.2e" % (rel_l2(gvp_f, gvp_e), rel_l2(grho_f, grho_e)))
    assert rel_l2(gvp_f, gvp_e) <= TOL_GRAD and rel_l2(grho_f, grho_e) <= TOL_GRAD
    assert gvs_e is not None and not gvs_e.any()


def test_checkpointed_equals_resident_and_calls_repeat():
    """nt = 90 in three checkpoint segments: the same bits as with resident snapshots, traces and gradients; and a second
    identical call returns the bits of the first."""
    from physicsbasedfwi2_amd import fluid
    c = _case(37, 70, 1, nt=90, seed=9)
    pl = fluid.FluidPlan(37, 70, 90, 3, 1, 13, 1, 6, 0, 0, 1, 1, 4)
    step_bytes = 4 * pl.layout.snap_step_elems
    pl.close()
    rng = np.random.default_rng(3)
    runs = []
    for budget in (None, None, 2 * 30 * step_bytes):
        mat, f, out = _run_hip(c, 1, 4, gs=2, budget=budget)
        if not runs:
            g = [(rng.standard_normal(tuple(a.shape)) * float(a.detach().abs().max())).astype(np.float32) for a in out]
        _backward(out, g)
        runs.append([a.detach().cpu().numpy() for a in out] + [mat.grad.cpu().numpy(), f.grad.cpu().numpy()])
    assert all(np.abs(a).max() > 0 for a in runs[0])
    for other, what in ((runs[1], "repeated call"), (runs[2], "three checkpoint segments")):
        for a, b in zip(runs[0], other):
            assert np.array_equal(a, b), what


def test_segment_count_of_the_checkpointed_run():
    """The budget of the test above does cut nt = 90 into three segments of 30."""
    from physicsbasedfwi2_amd import fluid
    from physicsbasedfwi2_amd._driver import checkpoint_schedule, segment_length
    pl = fluid.FluidPlan(37, 70, 90, 3, 1, 13, 1, 6, 0, 0, 1, 1, 4)
    step_bytes = 4 * pl.layout.snap_step_elems
    pl.close()
    seg = segment_length(2 * 30 * step_bytes, torch.device(DEV), step_bytes, 90)
    assert seg == 30 and len(checkpoint_schedule(90, seg, "elastic")[0]) == 3


def test_einval():
    """What the C-ABI refuses: fd_order, source_type, a free surface on fewer than 3 rows, null pointers, bad ranges."""
    import ctypes
    from physicsbasedfwi2_amd import _lib
    lib = _lib.load()
    base = dict(nz=20, nx=30, nt=10, nshot=1, nsrc=1, nrec=1, ntap=1, pml_width=0, free_surface=0, shots_per_group=0,
                source_type=0, fd_order=4)
    for bad in (dict(fd_order=3), dict(fd_order=8), dict(source_type=3), dict(source_type=-1), dict(free_surface=1, nz=2),
                dict(ntap=2), dict(pml_width=12)):
        h = ctypes.c_void_p()
        d = _lib.FluidDesc(**dict(base, **bad))
        assert lib.mifwi_fluid_plan_create(ctypes.byref(h), 0, ctypes.byref(d)) == -1, bad
    h = ctypes.c_void_p()
    d = _lib.FluidDesc(**dict(base, fd_order=0, free_surface=1, nz=3))
    assert lib.mifwi_fluid_plan_create(ctypes.byref(h), 0, ctypes.byref(d)) == 0
    lay = _lib.FluidLayout()
    assert lib.mifwi_fluid_plan_layout(h, ctypes.byref(lay)) == 0 and lay.gp == 32
    assert lib.mifwi_fluid_plan_cluster_slabs(h, 0) == 0 and lib.mifwi_fluid_plan_cluster_slabs(h, 1) == 0
    work = torch.zeros(max(lay.work_forward_elems, lay.work_backward_elems), device=DEV)
    buf = torch.zeros(4096, device=DEV)
    w, b = _lib.ptr(work), _lib.ptr(buf)
    fwd = lambda mat, wk, nb, ne, rvx=None, rvz=None: lib.mifwi_fluid_forward(
        h, mat, b, b, b, b, b, b, b, rvx, rvz, None, None, wk, nb, ne, 1, None)
    assert fwd(None, w, 0, 10) == -1 and fwd(b, None, 0, 10) == -1            # required pointers
    assert fwd(b, w, -1, 10) == -1 and fwd(b, w, 0, 11) == -1 and fwd(b, w, 5, 4) == -1
    assert fwd(b, w, 0, 10, rvx=b) == -1                                        # one velocity output without the other
    bwd = lambda snap, hi, lo, first=0, flags=1: lib.mifwi_fluid_backward(
        h, b, b, b, b, b, b, b, None, None, None, snap, first, None, None, w, hi, lo, flags, None)
    assert bwd(None, 9, 0) == -1 and bwd(b, 10, 0) == -1 and bwd(b, 9, -1) == -1
    assert bwd(b, 9, 0, first=1) == -1                                          # the snapshots start after the step needed
    assert bwd(b, 9, 0, flags=3) == -1                                          # finalize without grad_mat
    assert lib.mifwi_fluid_plan_destroy(h) == 0


# ---- the pyapi_denise switch --------------------------------------------------------------------------------------
def _denise(tmp_path, free_surf):
    import physicsbasedfwi2_amd.compat.pyapi_denise as api
    rng = np.random.default_rng(3)
    nz, nx, dx = 60, 90, 20.0
    vp = (1800 + 1200 * rng.random((nz, nx))).astype(np.float32)
    rho = (1900 + 300 * rng.random((nz, nx))).astype(np.float32)
    d = api.Denise("/nonexistent", verbose=0)
    d.save_folder = str(tmp_path)
    d.PHYSICS, d.ITERMAX = 2, 1
    d.TIME, d.DT, d.FREE_SURF, d.FW, d.FPML, d.DAMPING = 0.4, 0.002, free_surf, 10, 5.0, 1500.0
    xsrc = np.array([400.0, 1000.0, 1400.0])
    src = api.Sources(xsrc, 60.0 * xsrc / xsrc, 8.0)
    xrec = np.arange(300.0, 1500.0 + dx, 40.0)
    rec = api.Receivers(xrec, 460.0 * (xrec / xrec))
    mk = lambda s: api.Model(np.flipud(vp * s), np.flipud(np.zeros_like(vp)), np.flipud(rho), dx)
    return api, d, mk, src, rec


def _both_routes(d, model, src, rec):
    out = {}
    for route in ("elastic", "fluid"):
        d.acoustic_kernels = route
        loss = d.grad(model, src, rec)
        out[route] = (loss, d.get_fwi_gradients(["seis"]))
    (le, ge), (lf, gf) = out["elastic"], out["fluid"]
    print("loss elastic %.6e fluid %.6e; gradient rel-L2 rho %.2e vp %.2e" % (le, lf, rel_l2(gf[0], ge[0]), rel_l2(gf[1], ge[1])))
    assert le > 0 and abs(lf - le) <= 1e-6 * le
    assert np.abs(ge[0]).max() > 0 and np.abs(ge[1]).max() > 0
    assert rel_l2(gf[0], ge[0]) <= TOL_GRAD and rel_l2(gf[1], ge[1]) <= TOL_GRAD
    assert not gf[2].any() and not ge[2].any()                 # g_vs = 0 on both routes


def test_shim_grad_pressure_objective(tmp_path, monkeypatch):
    """PHYSICS = 2, QUELLTYP = 2 (force x), SEISMO = 4, QUELLTYPB = 4 under a free surface: d.grad through the fluid
    kernels against the elastic kernels."""
    api, d, mk, src, rec = _denise(tmp_path, 1)
    monkeypatch.chdir(tmp_path)
    d.QUELLTYP, d.SEISMO, d.QUELLTYPB = 2, 4, 4
    ox, oy = d.forward(mk(1.03), src, rec)
    op = np.stack(d.get_shots(keys=["_p"]))
    d.acoustic_kernels = "fluid"
    fx, fy = d.forward(mk(1.03), src, rec)
    fp = np.stack(d.get_shots(keys=["_p"]))
    assert np.abs(op).max() > 0
    assert rel_l2(fx, ox) <= TOL_TRACE and rel_l2(fy, oy) <= TOL_TRACE and rel_l2(fp, op) <= TOL_TRACE
    tr = lambda a: np.transpose(a, (0, 2, 1))
    d.set_observed(tr(ox), tr(oy), p=tr(op))
    _both_routes(d, mk(1.0), src, rec)


def test_shim_grad_stage_filter_trace_kill_and_impedance(tmp_path, monkeypatch):
    """The stage filter, a trace-kill table and INVMAT1 = 2 on the velocity objective, no free surface."""
    api, d, mk, src, rec = _denise(tmp_path, 0)
    monkeypatch.chdir(tmp_path)
    d.QUELLTYP, d.SEISMO, d.QUELLTYPB, d.INVMAT1 = 2, 1, 1, 2
    ox, oy = d.forward(mk(1.03), src, rec)
    d.acoustic_kernels = "fluid"
    fx, fy = d.forward(mk(1.03), src, rec)
    assert np.abs(ox).max() > 0 and np.array_equal(fx, ox) and np.array_equal(fy, oy)
    tr = lambda a: np.transpose(a, (0, 2, 1))
    d.set_observed(tr(ox), tr(oy))
    d.add_fwi_stage(fc_low=2.0, fc_high=12.0)
    table = np.zeros((len(rec), 3))
    table[3, 0] = table[7, 1] = table[8, 1] = table[-1, 2] = 1
    d.TRKILL = 1
    d.set_trace_kill(table)
    _both_routes(d, mk(1.0), src, rec)
