"""The fluid (variable-density acoustic) propagator at its edges: C-PML strips that cover the whole grid, no layer,
one to three time steps, dead taps, empty point sets, more points than threads, many taps per cell, shot counts against
the automatic group size, pass splitting with checkpointing, which inputs ask for gradients, NULL adjoint sources through
the C ABI.  Reference and bounds as in tests/test_fluid_gpu.py (cases.fluid_check): the f32 oracle of the elastic scheme on
mat5 = [K, K, 0, bx, bz], traces bit for bit, gradients to rel-L2 <= 2e-5, and every case first required to keep the f32
oracle's gL + gM within a quarter of that of the f64 oracle's.  Under a free surface sources sit on rows >= 1."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from cases import (elastic_case, fluid_backward, fluid_bits, fluid_check, fluid_oracle, fluid_planes, fluid_precondition,
                   fluid_run, fluid_sources_off_the_surface)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = ("rec_vx", "rec_vz", "rec_p", "grad_mat", "grad_f")


def _same_bits(a, b, what):
    for name, x, y in zip(NAMES, a, b):
        assert np.array_equal(x, y), (what, name)


# ---- (a) strips that cover the whole grid, no layer, other widths ------------------------------------------------------
# nz, nx, fw, free surface, steps.  W = fw + 1 nodes per side, wl = round_up(W, 4), xr0 = 4 * ((nx - W) // 4).
STRIP_GRIDS = [
    (8, 9, 3, 0, 40),        # W = 4 = wl = xr0 and 2 W = nz: every group and every row in a strip
    (8, 9, 3, 1, 40),
    (14, 15, 6, 0, 40),      # W = 7, wl = 8 = xr0, nx % 4 = 3
    (14, 17, 6, 0, 40),      # the right strip starts two columns before the layer
    (5, 9, 0, 0, 40),        # no layer
    (5, 9, 0, 1, 12),
    (24, 43, 9, 0, 40),      # W = 10, wl = 12
    (30, 47, 11, 0, 40),     # W = 12 = wl
]


@functools.lru_cache(maxsize=None)
def _strip_case(nz, nx, fw, fs, nt):
    c = elastic_case(seed=77, nz=nz, nx=nx, fw=fw, nt=nt, ns=2, nsrc=1, nrec=5, water=0, free_surface=bool(fs))
    if fs:      # shot 0 records on the surface row (rec_p = 0 there), shot 1 on row 1
        c["rc"][1] = c["rc"][0] + nx
        fluid_sources_off_the_surface(c)
    return fluid_planes(c, fs)


@functools.lru_cache(maxsize=None)
def _strip_oracle(grid, st, order):
    return fluid_oracle(_strip_case(*grid), st, order)


@pytest.mark.parametrize("grid", STRIP_GRIDS, ids=lambda g: "%dx%d-fw%d-fs%d" % g[:4])
@pytest.mark.parametrize("order", (2, 4))
@pytest.mark.parametrize("st", (0, 1, 2))
def test_strips_over_the_whole_grid_and_no_layer(grid, order, st):
    fluid_check(_strip_case(*grid), _strip_oracle(grid, st, order), st, order)


@pytest.mark.parametrize("fw", (3, 6, 9, 11))
def test_plan_refuses_grids_too_small_for_the_layer(fw):
    """2 W rows and wl + W columns is the smallest grid of a width (for fw = 3: 8 x 8; one column group less is 8 x 7);
    one row or one column less is refused."""
    from physicsbasedfwi2_amd import _lib
    lib = _lib.load()
    W = fw + 1
    wl = 4 * ((W + 3) // 4)
    base = dict(nt=10, nshot=1, nsrc=1, nrec=1, ntap=1, pml_width=fw, free_surface=0, shots_per_group=0, source_type=0,
                fd_order=4)
    for nz, nx, rc in ((2 * W, wl + W, 0), (2 * W - 1, wl + W + 1, -1), (2 * W, wl + W - 1, -1)):
        h = ctypes.c_void_p()
        d = _lib.FluidDesc(nz=nz, nx=nx, **base)
        assert lib.mifwi_fluid_plan_create(ctypes.byref(h), 0, ctypes.byref(d)) == rc, (nz, nx)
        if rc == 0:
            assert lib.mifwi_fluid_plan_destroy(h) == 0
    if fw == 3:
        for nz, nx in ((7, 9), (8, 7)):
            h = ctypes.c_void_p()
            d = _lib.FluidDesc(nz=nz, nx=nx, **base)
            assert lib.mifwi_fluid_plan_create(ctypes.byref(h), 0, ctypes.byref(d)) == -1, (nz, nx)


# ---- (b) one, two and three steps --------------------------------------------------------------------------------------
# What one step cannot reach.  The V launch reads p = 0, so its derivatives (the snapshot planes of bx and bz) are 0 and
# only a point force moves a velocity, the one it acts on; the P launch then builds p from that velocity, or from the
# explosive source alone (its snapshot plane, e1 + e2 of the velocities, is then 0).
ONE_STEP_ZERO = {0: ("rec_vx", "rec_vz", "gK", "gbx", "gbz"), 1: ("rec_vz", "gbx", "gbz"), 2: ("rec_vx", "gbx", "gbz")}


@functools.lru_cache(maxsize=None)
def _few_steps_case(nt, fs):
    nz, nx = 24, 21
    c = elastic_case(seed=79, nz=nz, nx=nx, fw=4, nt=nt, ns=1, nsrc=1, nrec=4, water=0, free_surface=bool(fs))
    c["f"] = np.full((nt, 1, 1), 1e6)
    src = 3 * nx + 10
    c["sc"] = np.array([[[src]]], dtype=np.int32)
    c["sw"] = np.ones((1, 1, 1))
    c["rc"] = np.array([[[src], [src + 1], [src + nx], [src - nx - 1]]], dtype=np.int32)
    c["rw"] = np.ones((1, 4, 1))
    return fluid_planes(c, fs)


@pytest.mark.parametrize("nt", (1, 2, 3))
@pytest.mark.parametrize("st", (0, 1, 2))
@pytest.mark.parametrize("fs", (0, 1))
def test_one_two_and_three_steps(nt, st, fs):
    """From two steps on nothing is zero; after one step what the step cannot reach is exactly zero, and rec_p and grad_f
    are not."""
    c = _few_steps_case(nt, fs)
    fluid_check(c, fluid_oracle(c, st, 4, g="ones"), st, 4, zero=ONE_STEP_ZERO[st] if nt == 1 else ())


# ---- (c) dead taps -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _dead_case(fs):
    c = elastic_case(seed=78, nz=44, nx=63, fw=8, nt=70, ns=3, nsrc=2, nrec=9, water=0, free_surface=bool(fs))
    if fs:
        fluid_sources_off_the_surface(c)
    c["sc"][0, 1, 0] = -1          # one dead source of shot 0
    c["sc"][2, :, 0] = -1          # shot 2: every source dead (an empty bounding box)
    c["rc"][:, 3, 0] = -1          # receiver 3 dead in every shot
    return fluid_planes(c, fs)


@pytest.mark.parametrize("st,fs", [(0, 0), (2, 1)])
def test_dead_taps_read_zero_and_inject_nothing(st, fs):
    c = _dead_case(fs)
    ref = fluid_oracle(c, st, 4)
    assert all(g[:, :, 3].all() for g in ref[1])          # a non-zero adjoint source on the dead receiver too
    _, (rvx, rvz, rp, _, gf) = fluid_check(c, ref, st, 4)
    for name, a in zip(NAMES, (rvx, rvz, rp)):
        assert not a[:, :, 3].any(), name + " of the dead receiver"
        assert not a[:, 2].any(), name + " of the shot without a source"
    assert gf[:, 0, 0].any() and gf[:, 1].any()
    assert not gf[:, 0, 1].any() and not gf[:, 2].any()


# ---- (d) empty point sets ----------------------------------------------------------------------------------------------
def test_no_receivers_or_no_sources():
    c = fluid_planes(elastic_case(seed=92, nz=30, nx=40, fw=4, nt=20, ns=2, nrec=3, water=0), 0)
    none_r = dict(c, rc=c["rc"][:, :0], rw=c["rw"][:, :0])
    for pressure in (False, True):
        mat, f, out = fluid_run(none_r, 0, 4, record_pressure=pressure)
        assert len(out) == 2 + pressure and all(tuple(a.shape) == (20, 2, 0) for a in out)
        torch.autograd.backward(list(out), [torch.zeros_like(a) for a in out])
        assert tuple(mat.grad.shape) == (3, 30, 40) and not mat.grad.cpu().numpy().any()
    none_s = dict(c, sc=c["sc"][:, :0], sw=c["sw"][:, :0], f=c["f"][:, :, :0])
    for st in (0, 1):
        mat, f, out = fluid_run(none_s, st, 4)
        assert all(tuple(a.shape) == (20, 2, 3) and not a.detach().cpu().numpy().any() for a in out)
        torch.autograd.backward(list(out), [torch.ones_like(a) for a in out])
        assert not mat.grad.cpu().numpy().any() and tuple(f.grad.shape) == (20, 2, 0)


# ---- (e) more points than threads, many taps per cell -------------------------------------------------------------------
MANY = dict(nz=30, nx=43, fw=4, nt=40, ns=3, water=0)      # 11 groups per row: one tile column forward and adjoint


@functools.lru_cache(maxsize=None)
def _many_receivers_case(fs):
    nz, nx = MANY["nz"], MANY["nx"]
    c = elastic_case(seed=76, nrec=700, free_surface=bool(fs), **MANY)
    if fs:
        fluid_sources_off_the_surface(c)
    rc = np.random.default_rng(1).integers(0, nz * nx, size=c["rc"].shape).astype(np.int32)
    rc[0, :5, 0] = [0, nx - 1, (nz - 1) * nx, nz * nx - 1, nx + 1]
    c["rc"], c["rw"] = rc, np.ones(rc.shape)
    return fluid_planes(c, fs)


@pytest.mark.parametrize("st,fs", [(0, 0), (2, 1)])
def test_more_receivers_than_threads_many_per_cell(st, fs):
    """700 receivers per shot on random cells (three sampling rows of fl_step_p, hundreds of taps per adjoint tile, several
    on one cell): traces bit for bit; the adjoint sources of a cell add in hardware order, so the gradients are held to the
    5e-5 of the elastic sibling in test_edge_cases_gpu.py.  Measured on an MI355X, where the order and so the figure
    changes from run to run: the largest rel-L2 of the four gradients was 3.7e-7 (explosive) and 7.1e-7 (fz under a free
    surface) over two runs, against that bound of 5e-5."""
    from physicsbasedfwi2_amd import fluid
    c = _many_receivers_case(fs)
    ref = fluid_oracle(c, st, 4)
    fluid_precondition(c, ref)
    pl = fluid.FluidPlan(30, 43, 40, 3, 1, 700, 1, 4, 0, 0, fs, st, 4)
    assert pl.layout.shots_per_group == 3 and pl.layout.ngroups == 1
    pl.close()
    errs, _ = fluid_check(c, ref, st, 4, tol=5e-5)
    print("700 receivers: largest gradient rel-L2 %.2e" % max(errs.values()))


@functools.lru_cache(maxsize=None)
def _many_sources_case(fs):
    nz, nx = MANY["nz"], MANY["nx"]
    c = elastic_case(seed=75, nsrc=300, nrec=9, free_surface=bool(fs), **MANY)
    rng = np.random.default_rng(2)
    first = nx if fs else 0
    sc = np.stack([first + rng.choice(nz * nx - first, 300, replace=False) for _ in range(3)])
    c["sc"], c["sw"] = sc[:, :, None].astype(np.int32), np.ones((3, 300, 1))
    assert all(len(set(s)) == 300 for s in sc) and (sc // nx >= (1 if fs else 0)).all()
    return fluid_planes(c, fs)


@pytest.mark.parametrize("st", (0, 2))
@pytest.mark.parametrize("fs", (0, 1))
def test_more_sources_than_threads(st, fs):
    """300 sources per shot on distinct cells, shots in groups of three: stage_injection's second round, and for the
    explosive source 900 > 256 samples of the adjoint pressure, the extra rows of fl_adj_p."""
    c = _many_sources_case(fs)
    fluid_check(c, fluid_oracle(c, st, 4), st, 4, gs=3)


# ---- (f) shot counts and automatic groups --------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _shots_case(ns, fs):
    c = elastic_case(seed=80 + ns, nz=30, nx=43, fw=4, nt=50, ns=ns, nsrc=1, nrec=9, water=0, free_surface=bool(fs))
    if fs:
        fluid_sources_off_the_surface(c)
    return fluid_planes(c, fs)


@pytest.mark.parametrize("ns,st,fs,gs,ngroups", [(6, 0, 0, 3, 2), (7, 1, 1, 4, 2), (1, 2, 0, 1, 1)])
def test_shot_counts_with_the_automatic_group_size(monkeypatch, ns, st, fs, gs, ngroups):
    """shots_per_group = 0: six shots go 3 + 3, seven 4 + 3 (a ragged last group), one alone.  Seven shots again in
    forward passes of two shots, adjoint passes of one group and three checkpoint segments: the bits of the plain run."""
    from physicsbasedfwi2_amd import fluid
    from physicsbasedfwi2_amd._driver import checkpoint_schedule, segment_length
    c = _shots_case(ns, fs)
    ref = fluid_oracle(c, st, 4)
    fluid_precondition(c, ref)
    pl = fluid.FluidPlan(30, 43, 50, ns, 1, 9, 1, 4, 0, 0, fs, st, 4)
    assert (pl.layout.shots_per_group, pl.layout.ngroups) == (gs, ngroups)
    step_bytes = 4 * pl.layout.snap_step_elems
    pl.close()
    _, plain = fluid_check(c, ref, st, 4)
    if ns != 7:
        return
    monkeypatch.setenv("MIFWI_FL_PASS_SHOTS", "2")
    monkeypatch.setenv("MIFWI_FL_PASS_GROUPS", "1")
    pl = fluid.FluidPlan(30, 43, 50, ns, 1, 9, 1, 4, 0, 0, fs, st, 4)
    assert pl.pass_sizes() == (2, 1)
    pl.close()
    budget = 2 * 17 * step_bytes
    seg = segment_length(budget, torch.device(DEV), step_bytes, 50)
    assert seg == 17 and len(checkpoint_schedule(50, seg, "elastic")[0]) == 3
    mat, f, out = fluid_run(c, st, 4, budget=budget)
    fluid_backward(out, ref[1])
    _same_bits(plain, fluid_bits(mat, f, out), "split passes and three checkpoint segments")


# ---- (g) which inputs ask for gradients ----------------------------------------------------------------------------------
def test_which_inputs_ask_for_gradients():
    """Only mat, only f: the bits of the run where both ask.  Without pressure receivers: the gradients of a run with them
    and g_p = 0."""
    from test_fluid_gpu import _case
    c = _case(37, 70, 1, nt=90, seed=9)
    rng = np.random.default_rng(6)
    mat, f, out = fluid_run(c, 1, 4)
    g = [(rng.standard_normal(tuple(a.shape)) * float(a.detach().abs().max())).astype(np.float32) for a in out]
    fluid_backward(out, g)
    both = fluid_bits(mat, f, out)
    assert all(np.abs(a).max() > 0 for a in both)
    mat, f, out = fluid_run(c, 1, 4, f_grad=False)
    fluid_backward(out, g)
    assert f.grad is None
    _same_bits(both[:4], [a.detach().cpu().numpy() for a in out] + [mat.grad.cpu().numpy()], "only mat asks")
    mat, f, out = fluid_run(c, 1, 4, mat_grad=False)
    fluid_backward(out, g)
    assert mat.grad is None
    _same_bits(both[:3] + both[4:], [a.detach().cpu().numpy() for a in out] + [f.grad.cpu().numpy()], "only f asks")
    g0 = g[:2] + [np.zeros_like(g[2])]
    mat, f, out = fluid_run(c, 1, 4)
    fluid_backward(out, g0)
    with_p = fluid_bits(mat, f, out)
    mat, f, out = fluid_run(c, 1, 4, record_pressure=False)
    assert len(out) == 2
    fluid_backward(out, g0)
    without_p = fluid_bits(mat, f, out)
    assert np.abs(with_p[3]).max() > 0 and np.abs(with_p[4]).max() > 0
    _same_bits(with_p[:2] + with_p[3:], without_p, "record_pressure=False against g_p = 0")


# ---- (h) NULL adjoint sources through the C ABI ----------------------------------------------------------------------------
@pytest.mark.parametrize("st", (0, 2))
def test_null_adjoint_sources_mean_zero(st):
    """include/mifwi.h: each of g_vx, g_vz, g_p NULL = zero; grad_f NULL: not computed, grad_mat unchanged."""
    from physicsbasedfwi2_amd import _lib, elastic
    lib = _lib.load()
    nz, nx, nt, nrec = 20, 30, 10, 3
    c = fluid_planes(elastic_case(seed=81, nz=nz, nx=nx, fw=0, nt=nt, ns=1, nsrc=1, nrec=nrec, water=0), 0)
    rng = np.random.default_rng(8)
    h = ctypes.c_void_p()
    d = _lib.FluidDesc(nz=nz, nx=nx, nt=nt, nshot=1, nsrc=1, nrec=nrec, ntap=1, pml_width=0, free_surface=0,
                       shots_per_group=0, source_type=st, fd_order=4)
    assert lib.mifwi_fluid_plan_create(ctypes.byref(h), 0, ctypes.byref(d)) == 0
    lay = _lib.FluidLayout()
    assert lib.mifwi_fluid_plan_layout(h, ctypes.byref(lay)) == 0 and lay.gp == 32
    dev = lambda a, dt=torch.float32: torch.tensor(np.asarray(a), dtype=dt, device=DEV)
    mat, pz, px = elastic._padded_inputs(dev(c["mat3"]), torch.tensor(c["pz"]), torch.tensor(c["px"]), lay.gp)
    src = int(c["sc"][0, 0, 0])
    sc, sw = dev(c["sc"], torch.int32), dev(c["sw"])
    rc, rw = dev([[[src + 1], [src + nx], [src - nx - 1]]], torch.int32), dev(np.ones((1, nrec, 1)))
    f = dev(1e6 * rng.standard_normal((nt, 1, 1)))
    P = _lib.ptr
    coef, geo = (P(mat), P(pz), P(px)), (P(sc), P(sw), P(rc), P(rw))
    snap = torch.empty(nt * lay.snap_step_elems, device=DEV)
    work = torch.empty(lay.work_forward_elems, device=DEV)
    rec = [torch.empty((nt, 1, nrec), device=DEV) for _ in range(3)]
    assert lib.mifwi_fluid_forward(h, *coef, P(f), *geo, *[P(a) for a in rec], P(snap), P(work), 0, nt,
                                   _lib.ZERO_STATE, None) == 0
    assert all(a.abs().max().item() > 0 for a in rec)
    gvx, gvz, gp = (dev(rng.standard_normal((nt, 1, nrec)) * a.abs().max().item()) for a in rec)
    zeros = torch.zeros_like(gvx)

    def adjoint(g_vx, g_vz, g_p, want_f=True):
        wk = torch.empty(lay.work_backward_elems, device=DEV)
        gm = torch.full((3, nz, lay.gp), float("nan"), device=DEV)
        gf = torch.zeros((nt, 1, 1), device=DEV) if want_f else None
        assert lib.mifwi_fluid_backward(h, *coef, *geo, P(g_vx), P(g_vz), P(g_p), P(snap), 0, P(gm), P(gf), P(wk), nt - 1, 0,
                                        _lib.ZERO_STATE | _lib.FINALIZE, None) == 0
        gm, gf = gm.cpu().numpy(), None if gf is None else gf.cpu().numpy()
        assert np.abs(gm[:, :, :nx]).max() > 0 and np.isfinite(gm).all() and (gf is None or np.abs(gf).max() > 0)
        return gm, gf

    for given, spelt in (((gvx, gvz, None), (gvx, gvz, zeros)), ((None, None, gp), (zeros, zeros, gp)),
                         ((gvx, None, None), (gvx, zeros, None))):
        (gm_a, gf_a), (gm_b, gf_b) = adjoint(*given), adjoint(*spelt)
        assert np.array_equal(gm_a, gm_b) and np.array_equal(gf_a, gf_b), [x is None for x in given]
    gm_a, _ = adjoint(gvx, gvz, gp)
    gm_b, _ = adjoint(gvx, gvz, gp, want_f=False)
    assert np.array_equal(gm_a, gm_b), "grad_f = NULL"
    assert lib.mifwi_fluid_plan_destroy(h) == 0


# ---- (i) bad cells -----------------------------------------------------------------------------------------------------
def test_a_receiver_outside_the_grid_fails_loudly():
    from physicsbasedfwi2_amd._lib import MifwiError
    c = fluid_planes(elastic_case(seed=77, nz=20, nx=24, fw=2, nt=5, ns=1, nrec=2, water=0), 0)
    c["rc"][0, 0, 0] = 20 * 24
    with pytest.raises(MifwiError):
        fluid_run(c, 0, 4)
