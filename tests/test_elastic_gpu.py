"""HIP elastic propagator vs the CPU oracle (fp32) on identical seeded inputs.

Same fmaf chain on both sides: seismograms are required to agree to rel-L2 <= 1e-6 (and are
reported bitwise); material gradients accumulate over time/shots in a different order:
rel-L2 <= 2e-5 per material plane.
"""
import numpy as np
import pytest
import torch

from cases import elastic_case, rel_l2

pytestmark = pytest.mark.gpu
TOL_TRACE = 1e-6
TOL_GRAD = 2e-5


def _run_hip(case, gs=0, budget=None, need_f=True, source_type="explosive", fd_order=4):
    from physicsbasedfwi2_amd import elastic
    dev = torch.device("cuda:0")
    mat = torch.tensor(case["mat"], dtype=torch.float32, device=dev, requires_grad=True)
    f = torch.tensor(case["f"], dtype=torch.float32, device=dev, requires_grad=need_f)
    kw = {} if budget is None else {"snapshot_budget": budget}
    rvx, rvz = elastic.propagate(mat, f, torch.tensor(case["pz"]), torch.tensor(case["px"]),
                                 torch.tensor(case["sc"]), torch.tensor(case["sw"]),
                                 torch.tensor(case["rc"]), torch.tensor(case["rw"]),
                                 case["fw"], shots_per_group=gs, free_surface=bool(case["fs"]),
                                 source_type=source_type, fd_order=fd_order, **kw)
    return mat, f, rvx, rvz


@pytest.mark.parametrize("kw", [
    dict(),
    dict(nz=37, nx=53, fw=6, ns=3, nrec=11),              # ragged sizes
    dict(nz=70, nx=300, fw=10, ns=2, nrec=30, nt=80),     # reference grid width, LX=64
    dict(nz=50, nx=66, fw=0, water=0),                     # no absorbing layer at all
    dict(free_surface=True),                               # stress-imaging free surface, water on top
    dict(free_surface=True, water=0, nz=37, nx=53, fw=6),  # free surface on a solid, ragged sizes
])
def test_forward_backward_parity(oracle32, kw):
    _check_parity(oracle32, elastic_case(seed=4, **kw))


def _check_parity(o, case, bitwise=False, source_type=0, fd_order=4):
    ovx, ovz, S = o.elastic_forward(case["mat"], case["pz"], case["px"], case["f"], case["sc"],
                                    case["sw"], case["rc"], case["rw"], save=True,
                                    free_surface=case["fs"], source_type=source_type, fd_order=fd_order)
    mat, f, rvx, rvz = _run_hip(case, source_type=source_type, fd_order=fd_order)
    hx, hz = rvx.detach().cpu().numpy(), rvz.detach().cpu().numpy()
    assert np.isfinite(hx).all() and np.abs(ovx).max() > 0 and np.abs(ovz).max() > 0
    print("max |hip-oracle| vx %.3e vz %.3e" % (np.abs(hx - ovx).max(), np.abs(hz - ovz).max()))
    assert rel_l2(hx, ovx) <= TOL_TRACE and rel_l2(hz, ovz) <= TOL_TRACE
    if bitwise:
        assert np.abs(hx - ovx).max() == 0.0 and np.abs(hz - ovz).max() == 0.0
    rng = np.random.default_rng(12)
    gx = (rng.standard_normal(ovx.shape) * np.abs(ovx).max()).astype(np.float32)
    gz = (rng.standard_normal(ovz.shape) * np.abs(ovz).max()).astype(np.float32)
    torch.autograd.backward([rvx, rvz], [torch.tensor(gx, device=rvx.device),
                                         torch.tensor(gz, device=rvx.device)])
    gm_o, gf_o = o.elastic_backward(case["mat"], case["pz"], case["px"], case["sc"], case["sw"],
                                    case["rc"], case["rw"], gx, gz, S, free_surface=case["fs"],
                                    source_type=source_type, fd_order=fd_order)
    gm_h = mat.grad.cpu().numpy()
    for k, name in enumerate(["lambda", "lambda+2mu", "mu_xz", "1/rho_x", "1/rho_z"]):
        assert rel_l2(gm_h[k], gm_o[k]) <= TOL_GRAD, name
    assert rel_l2(f.grad.cpu().numpy(), gf_o) <= TOL_GRAD


@pytest.mark.parametrize("nw,fs", [(2, False), (3, True), (5, False), (7, True)])
def test_cluster_path_with_halo_handoff(oracle32, monkeypatch, nw, fs):
    """Force the LDS-resident cluster kernel to cut a shot into several row slabs so that the
    velocity/stress granule hand-off between workgroups is exercised: traces stay bitwise equal
    to the oracle and the snapshot stream (checked through the gradients) is unchanged."""
    monkeypatch.setenv("MIFWI_EL_NW", str(nw))          # forward and adjoint kernels alike
    case = elastic_case(seed=23, nz=61, nx=83, fw=8, ns=3, nrec=15, nt=120, free_surface=fs)
    _check_parity(oracle32, case, bitwise=True)


def test_cluster_path_without_absorbing_layer(oracle32, monkeypatch):
    """No C-PML at all (W = 0: no memory variables, no strip tables) on several slabs."""
    monkeypatch.setenv("MIFWI_EL_NW", "4")
    _check_parity(oracle32, elastic_case(seed=39, nz=50, nx=66, fw=0, water=0, nt=90), bitwise=True)


def test_cluster_path_on_the_widest_reference_grid_width(oracle32):
    """nx = 396 (the 170x396 grid of networks.py:8224): 99 groups per row, ten-row slabs."""
    case = elastic_case(seed=37, nz=64, nx=396, fw=10, ns=2, nrec=50, nt=100)
    _check_parity(oracle32, case, bitwise=True)


def test_cluster_adjoint_receivers_everywhere(oracle32, monkeypatch):
    """Receivers in several slabs and several per 4-cell group; two sources in one group."""
    monkeypatch.setenv("MIFWI_EL_NW", "4")
    case = elastic_case(seed=31, nz=48, nx=64, fw=6, ns=2, nsrc=2, nrec=64, nt=90)
    nz, nx = 48, 64
    rng = np.random.default_rng(5)
    rc = rng.choice(nz * nx, size=(2, 64), replace=False).astype(np.int32)
    rc[:, :8] = (7 * nx + 20 + np.arange(8)).astype(np.int32)      # a run of neighbours on one row
    case["rc"] = rc.reshape(case["rc"].shape)
    sc = case["sc"].copy().reshape(2, 2)
    sc[:, 0] = 9 * nx + 30
    sc[:, 1] = 9 * nx + 31                                           # same group as the first source
    case["sc"] = sc.reshape(case["sc"].shape)
    _check_parity(oracle32, case)


@pytest.mark.parametrize("nz,nx,nw", [(45, 272, 3), (25, 64, 5), (24, 100, 6), (27, 83, 3), (52, 300, 4)],
                         ids=lambda v: str(v))
def test_cluster_group_dealing_shapes(oracle32, monkeypatch, nz, nx, nw):
    """How a slab's groups are dealt to the threads (ec_slot: interior groups first, boundary groups from the next wave
    boundary, interior groups of the second slot updated late) on shapes at its edges: two slots with no room for the
    pad (15 rows x 68 groups), five-row slabs (one interior row), four-row slabs (no interior row), a single slot, and
    13-row slabs of 75 groups as in 100x300.  Bitwise traces and 2e-5 gradients against the oracle; conftest fails the
    test if a time loop gave up and the per-step kernels produced the numbers."""
    from physicsbasedfwi2_amd.elastic import ElasticPlan
    monkeypatch.setenv("MIFWI_EL_NW", str(nw))
    pl = ElasticPlan(nz, nx, 60, 2, 1, 12, 1, 6, 0)
    assert pl.cluster_slabs(False) == nw and pl.cluster_slabs(True) == nw
    _check_parity(oracle32, elastic_case(seed=61 + nz, nz=nz, nx=nx, fw=6, ns=2, nrec=12, nt=60), bitwise=True)


@pytest.mark.parametrize("nz,nx,nw,expect", [(100, 300, 8, True), (52, 300, 4, True), (45, 272, 3, False), (24, 100, 6, None)],
                         ids=lambda v: str(v))
def test_cluster_lane_halo_form_equals_the_lds_reads(monkeypatch, nz, nx, nw, expect):
    """The single-launch kernels take the outer cells of their x-stencils from the neighbouring lanes (DPP wave shifts,
    ec_xhalo) where the deal of groups to lanes allows it - BASELINE config 3's 100x300 on 8 slabs does (layout.kernel_flags)
    - and from LDS otherwise (15 rows x 68 groups: boundary and late-interior groups meet inside a wave).  Data movement
    only: seismograms and gradients are the same bits as with MIFWI_EL_XHALO=0."""
    from physicsbasedfwi2_amd import _lib, elastic
    from physicsbasedfwi2_amd.elastic import ElasticPlan
    monkeypatch.setenv("MIFWI_EL_NW", str(nw))
    case = elastic_case(seed=77, nz=nz, nx=nx, fw=6, ns=2, nrec=12, nt=60)
    both = _lib.EL_KERNEL_FWD_LANE_HALO | _lib.EL_KERNEL_ADJ_LANE_HALO
    outs = []
    for flag in ("1", "0"):
        monkeypatch.setenv("MIFWI_EL_XHALO", flag)
        pl = ElasticPlan(nz, nx, 60, 2, 1, 12, 1, 6, 0)
        assert pl.cluster_slabs(False) == nw and pl.cluster_slabs(True) == nw
        got = pl.layout.kernel_flags & both
        pl.close()
        if flag == "0":
            assert got == 0
        elif expect is not None:
            assert got == (both if expect else 0), got
        dev = torch.device("cuda:0")
        mat = torch.tensor(case["mat"], dtype=torch.float32, device=dev, requires_grad=True)
        f = torch.tensor(case["f"], dtype=torch.float32, device=dev, requires_grad=True)
        rvx, rvz = elastic.propagate(mat, f, torch.tensor(case["pz"]), torch.tensor(case["px"]), torch.tensor(case["sc"]),
                                     torch.tensor(case["sw"]), torch.tensor(case["rc"]), torch.tensor(case["rw"]), case["fw"])
        (0.5 * (rvx ** 2).sum() + 0.5 * (rvz ** 2).sum()).backward()
        outs.append((rvx.detach().clone(), rvz.detach().clone(), mat.grad.clone(), f.grad.clone()))
    assert float(outs[0][0].abs().max()) > 0
    for a, b in zip(outs[0], outs[1]):
        assert torch.equal(a, b)


def test_cluster_adjoint_source_paths_agree(oracle32, monkeypatch):
    """The single-launch adjoint adds its sources through a receiver-row buffer (plain LDS stores) where every tap of a
    slab has a cell of its own on at most four rows, and through LDS float atomics otherwise (MIFWI_EL_ADJ_DIRECT=0
    forces them): same bits either way.  Two receivers sharing a cell must drop to the atomic path by themselves."""
    monkeypatch.setenv("MIFWI_EL_NW", "3")
    case = elastic_case(seed=53, nz=60, nx=100, fw=8, ns=2, nrec=60, nt=90)
    nx = 100
    rc = np.empty((2, 60), dtype=np.int32)
    rc[:, :30] = 12 * nx + 5 + 3 * np.arange(30)                  # two receiver rows in the first slab,
    rc[:, 30:50] = 15 * nx + 7 + 4 * np.arange(20)
    rc[:, 50:] = 33 * nx + 10 + 8 * np.arange(10)                 # one in the second
    case["rc"] = rc.reshape(case["rc"].shape)
    outs = []
    for flag in (None, "0"):
        if flag is not None:
            monkeypatch.setenv("MIFWI_EL_ADJ_DIRECT", flag)
        mat, f, rvx, rvz = _run_hip(case)
        torch.autograd.backward([rvx, rvz], [torch.sign(rvx.detach()), torch.sign(rvz.detach())])
        outs.append((mat.grad.clone(), f.grad.clone()))
    assert float(outs[0][0].abs().max()) > 0
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    monkeypatch.delenv("MIFWI_EL_ADJ_DIRECT")
    _check_parity(oracle32, case, bitwise=True)
    rc[:, 1] = rc[:, 0]                                           # two taps in one cell
    case["rc"] = rc.reshape(case["rc"].shape)
    _check_parity(oracle32, case, bitwise=True)


def test_cluster_and_per_step_paths_agree(monkeypatch):
    case = elastic_case(seed=29, nz=70, nx=300, fw=10, ns=2, nrec=40, nt=100)   # two groups per thread
    outs = []
    for flag in ("1", "0"):
        monkeypatch.setenv("MIFWI_EL_CLUSTER", flag)
        monkeypatch.setenv("MIFWI_EL_CLUSTER_ADJ", flag)
        mat, f, rvx, rvz = _run_hip(case)
        torch.autograd.backward([rvx, rvz], [torch.sign(rvx.detach()), torch.sign(rvz.detach())])
        outs.append((rvx.detach().clone(), rvz.detach().clone(), mat.grad.clone(), f.grad.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert rel_l2(outs[0][2].cpu().numpy(), outs[1][2].cpu().numpy()) <= TOL_GRAD
    assert rel_l2(outs[0][3].cpu().numpy(), outs[1][3].cpu().numpy()) <= TOL_GRAD


@pytest.mark.parametrize("gs", [1, 2, 3])
def test_shot_groups(oracle32, gs):
    case = elastic_case(seed=8, ns=5, nt=70)
    o = oracle32
    ovx, ovz, S = o.elastic_forward(case["mat"], case["pz"], case["px"], case["f"], case["sc"],
                                    case["sw"], case["rc"], case["rw"], save=True)
    mat, f, rvx, rvz = _run_hip(case, gs=gs)
    assert rel_l2(rvx.detach().cpu().numpy(), ovx) <= TOL_TRACE
    gx, gz = np.sign(ovx).astype(np.float32), np.sign(ovz).astype(np.float32)
    torch.autograd.backward([rvx, rvz], [torch.tensor(gx, device=rvx.device),
                                         torch.tensor(gz, device=rvx.device)])
    gm_o, gf_o = o.elastic_backward(case["mat"], case["pz"], case["px"], case["sc"], case["sw"],
                                    case["rc"], case["rw"], gx, gz, S)
    gm_h = mat.grad.cpu().numpy()
    for k in range(5):
        assert rel_l2(gm_h[k], gm_o[k]) <= TOL_GRAD
    assert rel_l2(f.grad.cpu().numpy(), gf_o) <= TOL_GRAD


def test_time_checkpointing_matches_resident_snapshots():
    case = elastic_case(seed=10, nt=90, ns=2)
    m1, f1, x1, z1 = _run_hip(case)
    gx, gz = torch.sign(x1.detach()), torch.sign(z1.detach())
    torch.autograd.backward([x1, z1], [gx, gz])
    nz, nx = case["mat"].shape[1:]
    step_bytes = 4 * 5 * 2 * nz * ((nx + 3) // 4 * 4)
    m2, f2, x2, z2 = _run_hip(case, budget=step_bytes * 2 * 11)
    torch.autograd.backward([x2, z2], [gx, gz])
    assert torch.equal(x1, x2) and torch.equal(z1, z2)
    assert torch.equal(m1.grad, m2.grad)
    assert torch.equal(f1.grad, f2.grad)


def test_determinism():
    case = elastic_case(seed=14, ns=3)
    outs = []
    for _ in range(2):
        m, f, x, z = _run_hip(case)
        torch.autograd.backward([x, z], [torch.ones_like(x), torch.ones_like(z)])
        outs.append((x.detach().clone(), z.detach().clone(), m.grad.clone(), f.grad.clone()))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_vp_vs_rho_chain(oracle32):
    """(vp, vs, rho) -> staggered materials -> propagator: torch autograd composes the host-side
    averaging with the HIP adjoint; compare with the same composition around the oracle."""
    from physicsbasedfwi2_amd import elastic
    case = elastic_case(seed=16, nt=100)
    dev = torch.device("cuda:0")
    prm = [torch.tensor(case[k], dtype=torch.float32, device=dev, requires_grad=True)
           for k in ("vp", "vs", "rho")]
    mat = elastic.staggered_materials(*prm, case["dt"], case["h"])
    assert rel_l2(mat.detach().cpu().numpy(), case["mat"]) <= 1e-6
    rvx, rvz = elastic.propagate(mat, torch.tensor(case["f"], dtype=torch.float32, device=dev),
                                 torch.tensor(case["pz"]), torch.tensor(case["px"]),
                                 torch.tensor(case["sc"]), torch.tensor(case["sw"]),
                                 torch.tensor(case["rc"]), torch.tensor(case["rw"]), case["fw"])
    loss = 0.5 * (rvx ** 2).sum() + 0.5 * (rvz ** 2).sum()
    loss.backward()
    # oracle composition on the CPU
    prc = [torch.tensor(case[k], dtype=torch.float32, requires_grad=True)
           for k in ("vp", "vs", "rho")]
    mat_c = elastic.staggered_materials(*prc, case["dt"], case["h"])
    m_np = mat_c.detach().numpy()
    ovx, ovz, S = oracle32.elastic_forward(m_np, case["pz"], case["px"], case["f"], case["sc"],
                                           case["sw"], case["rc"], case["rw"], save=True)
    gm, _ = oracle32.elastic_backward(m_np, case["pz"], case["px"], case["sc"], case["sw"],
                                      case["rc"], case["rw"], ovx, ovz, S, want_grad_f=False)
    mat_c.backward(torch.tensor(gm))
    for a, b, name in zip(prm, prc, ("vp", "vs", "rho")):
        assert rel_l2(a.grad.cpu().numpy(), b.grad.numpy()) <= 5e-5, name


@pytest.mark.parametrize("source_type,kw", [
    (1, dict(nsrc=2)),
    (2, dict(nsrc=2, free_surface=True)),
    (2, dict(nz=100, nx=300, fw=10, ns=5, nrec=40, nt=60)),      # a grid the explosive source runs single-launch
])
def test_point_force_sources_parity(oracle32, source_type, kw):
    """desc.source_type 1 / 2: f goes into vx / vz between V and S (launches of their own on the per-step
    kernels); seismograms, material gradients and the source gradient against oracle/elastic.c."""
    case = elastic_case(seed=21, **kw)
    case["f"] = (case["f"] * 1e-3).astype(np.float32)
    _check_parity(oracle32, case, source_type=source_type)


def test_force_amplitude_carries_the_density_gradient():
    """elastic.force_amplitude scales the wavelet by dt/(h^2 rho) at the source node inside autograd: the
    gradient w.r.t. the buoyancy plane gets the source term's share (finite-difference check of that share)."""
    from physicsbasedfwi2_amd import elastic
    case = elastic_case(seed=23, nsrc=1, ns=2, nrec=12, nt=60)
    dev = torch.device("cuda:0")
    sc, sw = torch.tensor(case["sc"]), torch.tensor(case["sw"])
    geo = (torch.tensor(case["pz"]), torch.tensor(case["px"]), sc, sw, torch.tensor(case["rc"]), torch.tensor(case["rw"]))
    wav = torch.tensor(case["f"] * 1e-3, dtype=torch.float32, device=dev)

    def run(mat_amp, mat_prop):
        f = elastic.force_amplitude(wav, mat_amp, sc, sw, 20.0, "fz")
        vx, vz = elastic.propagate(mat_prop, f, *geo, case["fw"], source_type="fz")
        return 0.5 * (vx.double() ** 2).sum() + 0.5 * (vz.double() ** 2).sum()
    mat = torch.tensor(case["mat"], dtype=torch.float32, device=dev)
    m_amp = mat.clone().requires_grad_(True)
    J0 = run(m_amp, mat)                       # only the amplitude path sees m_amp
    J0.backward()
    cell = int(case["sc"][0, 0, 0])
    g = float(m_amp.grad[4].reshape(-1)[cell])
    assert g != 0.0 and float(m_amp.grad[3].abs().max()) == 0.0
    eps = 1e-2
    m2 = mat.clone()
    m2[4].view(-1)[cell] *= (1 + eps)
    fd = (float(run(m2, mat).detach()) - float(J0.detach())) / (eps * float(mat[4].reshape(-1)[cell]))
    assert abs(fd - g) <= 2e-2 * abs(g)


@pytest.mark.parametrize("kw", [dict(nsrc=2), dict(free_surface=True, nz=100, nx=300, fw=10, ns=5, nrec=40, nt=60)])
def test_pressure_receivers_parity(oracle32, kw):
    """record_pressure: rec_p = sum w (sxx + szz) after the stress update; the adjoint source goes into the adjoint
    sxx and szz before S^T.  Seismograms and all gradients of an objective on (vx, vz, p) against the oracle;
    the velocity seismograms of such a plan equal those of a plain one bit for bit."""
    from physicsbasedfwi2_amd import elastic
    case = elastic_case(seed=29, **kw)
    o, fs = oracle32, case["fs"]
    geo = (case["sc"], case["sw"], case["rc"], case["rw"])
    ovx, ovz, S, op = o.elastic_forward(case["mat"], case["pz"], case["px"], case["f"], *geo, save=True,
                                        free_surface=fs, pressure=True)
    dev = torch.device("cuda:0")
    mat = torch.tensor(case["mat"], dtype=torch.float32, device=dev, requires_grad=True)
    f = torch.tensor(case["f"], dtype=torch.float32, device=dev, requires_grad=True)
    tg = [torch.tensor(case[k]) for k in ("pz", "px", "sc", "sw", "rc", "rw")]
    rvx, rvz, rp = elastic.propagate(mat, f, *tg, case["fw"], free_surface=bool(fs), record_pressure=True)
    pvx, pvz = elastic.propagate(mat.detach(), f.detach(), *tg, case["fw"], free_surface=bool(fs))
    assert torch.equal(rvx.detach(), pvx) and torch.equal(rvz.detach(), pvz)
    assert np.abs(op).max() > 0 and rel_l2(rp.detach().cpu().numpy(), op) <= TOL_TRACE
    rng = np.random.default_rng(14)
    gx, gz, gp = ((rng.standard_normal(a.shape) * np.abs(a).max()).astype(np.float32) for a in (ovx, ovz, op))
    torch.autograd.backward([rvx, rvz, rp], [torch.tensor(g, device=dev) for g in (gx, gz, gp)])
    gm_o, gf_o = o.elastic_backward(case["mat"], case["pz"], case["px"], *geo, gx, gz, S, free_surface=fs, g_p=gp)
    for k in range(5):
        assert rel_l2(mat.grad[k].cpu().numpy(), gm_o[k]) <= TOL_GRAD, k
    assert rel_l2(f.grad.cpu().numpy(), gf_o) <= TOL_GRAD


def _bf16_round(a):
    """float32 -> bf16 -> float32, round to nearest even (what v_cvt_pk_bf16_f32 does to finite values)."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).reshape(np.shape(a))


@pytest.mark.parametrize("kw", [dict(nz=60, nx=150, fw=8, ns=3, nrec=21, nt=90),
                                dict(nz=37, nx=53, fw=6, ns=2, nrec=11, free_surface=True)])
def test_bf16_snapshot_planes(oracle32, monkeypatch, kw):
    """snapshot_format="bf16" (per-step kernels): the seismograms do not change; the gradient is the oracle's
    gradient computed from snapshot planes rounded to bf16 (<= 2e-5, so the only difference to the exact mode
    IS the rounding of the stored planes) and stays within 4e-3 rel-L2 of the exact gradient even for white-noise
    residuals over ~100 steps, where nothing averages out (each stored sample is off by at most 2^-9 = 2e-3);
    time checkpointing reproduces the resident run bit for bit; half the snapshot memory."""
    from physicsbasedfwi2_amd import _lib, elastic
    monkeypatch.setenv("MIFWI_EL_CLUSTER", "0")
    monkeypatch.setenv("MIFWI_EL_CLUSTER_ADJ", "0")
    case = elastic_case(seed=29, **kw)
    fs = case["fs"]
    nt, ns = case["f"].shape[:2]
    nz, nx = case["mat"].shape[1:]
    lay = {}
    for fmt in ("f32", "bf16"):
        pl = elastic.ElasticPlan(nz, nx, nt, ns, 1, case["rc"].shape[1], 1, case["fw"], 0, 0, fs, snapshot_format=fmt)
        lay[fmt] = (pl.layout.snapshot_format, pl.layout.snap_step_elems)
        pl.close()
    assert lay["f32"][0] == _lib.SNAPSHOT_F32 and lay["bf16"][0] == _lib.SNAPSHOT_BF16
    assert lay["bf16"][1] <= 0.5 * lay["f32"][1] + 4 * ns
    o = oracle32
    ovx, ovz, S = o.elastic_forward(case["mat"], case["pz"], case["px"], case["f"], case["sc"], case["sw"],
                                    case["rc"], case["rw"], save=True, free_surface=fs)
    rng = np.random.default_rng(12)
    gx = (rng.standard_normal(ovx.shape) * np.abs(ovx).max()).astype(np.float32)
    gz = (rng.standard_normal(ovz.shape) * np.abs(ovz).max()).astype(np.float32)
    dev = torch.device("cuda:0")

    def run(fmt, budget=None):
        mat = torch.tensor(case["mat"], dtype=torch.float32, device=dev, requires_grad=True)
        f = torch.tensor(case["f"], dtype=torch.float32, device=dev, requires_grad=True)
        kw2 = {} if budget is None else {"snapshot_budget": budget}
        rvx, rvz = elastic.propagate(mat, f, torch.tensor(case["pz"]), torch.tensor(case["px"]),
                                     torch.tensor(case["sc"]), torch.tensor(case["sw"]), torch.tensor(case["rc"]),
                                     torch.tensor(case["rw"]), case["fw"], free_surface=bool(fs),
                                     snapshot_format=fmt, **kw2)
        torch.autograd.backward([rvx, rvz], [torch.tensor(gx, device=dev), torch.tensor(gz, device=dev)])
        return rvx.detach(), rvz.detach(), mat.grad.clone(), f.grad.clone()
    ex = run("f32")
    bf = run("bf16")
    assert torch.equal(ex[0], bf[0]) and torch.equal(ex[1], bf[1])
    assert np.abs(bf[0].cpu().numpy() - ovx).max() == 0.0
    gm_exact, gf_o = o.elastic_backward(case["mat"], case["pz"], case["px"], case["sc"], case["sw"], case["rc"],
                                        case["rw"], gx, gz, S, free_surface=fs)
    gm_round, _ = o.elastic_backward(case["mat"], case["pz"], case["px"], case["sc"], case["sw"], case["rc"],
                                     case["rw"], gx, gz, _bf16_round(S), free_surface=fs)
    gh = bf[2].cpu().numpy()
    for k in range(5):
        assert rel_l2(gh[k], gm_round[k]) <= TOL_GRAD, k
        e = rel_l2(gh[k], gm_exact[k])
        assert 1e-6 < e <= 4e-3, (k, e)                      # rounded planes were used, and cost this much
    assert rel_l2(bf[3].cpu().numpy(), gf_o) <= TOL_GRAD     # the source gradient does not read the planes
    seg = run("bf16", budget=4 * lay["bf16"][1] * 2 * 17)     # 17-step segments
    for a, b in zip(bf, seg):
        assert torch.equal(a, b)


def test_bf16_request_on_a_single_launch_plan_keeps_f32():
    """Grids that run LDS-resident are not bound by the snapshot stream: the plan says so in its layout and
    the results are the exact ones."""
    from physicsbasedfwi2_amd import _lib, elastic
    pl = elastic.ElasticPlan(100, 300, 200, 6, 1, 200, 1, 10, 0, snapshot_format="bf16")
    assert pl.cluster_slabs(False) >= 1 and pl.layout.snapshot_format == _lib.SNAPSHOT_F32
    assert pl.layout.snap_step_elems == 5 * 6 * pl.layout.coef_elems
    pl.close()


@pytest.mark.parametrize("env", [
    {},                                                                                   # single-launch kernels
    {"MIFWI_EL_NW": "3"},                                                                 # ... with halo hand-off
    {"MIFWI_EL_CLUSTER": "0", "MIFWI_EL_CLUSTER_ADJ": "0"},                               # one launch per half step
    {"MIFWI_EL_CLUSTER": "0", "MIFWI_EL_CLUSTER_ADJ": "0", "MIFWI_EL_FUSED": "1"},        # ... fused forward
])
def test_second_order_stencils(oracle32, monkeypatch, env):
    """fd_order = 2 (DENISE FD_ORDER; weights (1, 0) in the four-point form) through every kernel family, with the
    free surface: seismograms bit for bit, gradients <= 2e-5 against the oracle run at the same order - and not
    the fourth-order answer."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    case = elastic_case(seed=31, nz=61, nx=83, fw=8, ns=3, nrec=15, nt=110, free_surface=True)
    _check_parity(oracle32, case, bitwise=True, fd_order=2)
    ovx4, _ = oracle32.elastic_forward(case["mat"], case["pz"], case["px"], case["f"], case["sc"], case["sw"],
                                       case["rc"], case["rw"], free_surface=1)
    _, _, rvx, _ = _run_hip(case, fd_order=2)
    assert rel_l2(rvx.detach().cpu().numpy(), ovx4) > 1e-3


def test_gradient_in_shot_chunks_equals_the_all_shots_gradient():
    """Shots are independent: taking them two at a time (each chunk forward with resident snapshots, straight into its
    adjoint) gives the loss and the material / wavelet gradients of the all-shots call - the cut that replaces time
    checkpointing when the misfit is known up front (elastic.gradient_in_shot_chunks)."""
    from physicsbasedfwi2_amd import elastic, misfit
    case = elastic_case(seed=97, nz=60, nx=150, fw=10, ns=5, nrec=40, nt=90)
    dev = "cuda:0"
    t = lambda n: torch.tensor(case[n])
    obs = [torch.randn(90, 5, 40, device=dev) * 1e-3 for _ in range(2)]

    def loss_fn(rvx, rvz, sl):
        return misfit.l2_half(rvx, obs[0][:, sl].contiguous()) + misfit.l2_half(rvz, obs[1][:, sl].contiguous())

    def run(chunk):
        mat = torch.tensor(case["mat"], dtype=torch.float32, device=dev, requires_grad=True)
        f = torch.tensor(case["f"], dtype=torch.float32, device=dev, requires_grad=True)
        args = (t("pz"), t("px"), t("sc"), t("sw"), t("rc"), t("rw"), case["fw"])
        if chunk:
            loss = elastic.gradient_in_shot_chunks(mat, f, *args, loss_fn, chunk)
        else:
            rvx, rvz = elastic.propagate(mat, f, *args)
            loss = loss_fn(rvx, rvz, slice(0, 5))
            loss.backward()
            loss = loss.detach()
        return float(loss), mat.grad.cpu().numpy(), f.grad.cpu().numpy()

    l0, gm0, gf0 = run(0)
    assert l0 > 0 and np.abs(gm0).max() > 0 and np.abs(gf0).max() > 0
    for chunk in (2, 5, 1):
        l1, gm1, gf1 = run(chunk)
        assert abs(l1 - l0) <= 1e-6 * l0
        assert rel_l2(gm1, gm0) <= 2e-6 and rel_l2(gf1, gf0) <= 2e-6
    assert elastic.resident_shot_chunk(32, 3000, 350, 1700) == 2        # 35.7 GB of f32 planes per shot, 96 GB budget
    assert elastic.resident_shot_chunk(32, 3000, 100, 300) == 32 and elastic.resident_shot_chunk(16, 5000, 1000, 3000) == 0


def test_snapshot_arena_has_one_owner_at_a_time():
    """Two forward passes inside one `elastic.snapshot_arena()` before either backward (two components, a forward
    inside a loss closure, retain_graph): the second must NOT be handed the tensor the first still needs - it gets
    snapshots of its own - and once a backward has consumed the arena's planes the next forward may reuse them.
    Gradients equal those of the same passes run without an arena, bit for bit."""
    from physicsbasedfwi2_amd import elastic
    ca = elastic_case(seed=101, nz=50, nx=90, fw=8, ns=3, nrec=20, nt=70)
    cb = elastic_case(seed=103, nz=50, nx=90, fw=8, ns=3, nrec=20, nt=70)

    def fwd(c):
        mat, f, rvx, rvz = _run_hip(c)
        return mat, f, rvx, rvz

    def grads(use_arena):
        import contextlib
        ctx = elastic.snapshot_arena() if use_arena else contextlib.nullcontext()
        with ctx as arena:
            ma, fa, ax, az = fwd(ca)
            mb, fb, bx, bz = fwd(cb)                              # before a's backward
            if use_arena:
                assert arena.busy()
            torch.autograd.backward([bx, bz], [torch.sign(bx.detach()), torch.sign(bz.detach())])
            torch.autograd.backward([ax, az], [torch.sign(ax.detach()), torch.sign(az.detach())])
            if use_arena:
                assert not arena.busy()                           # a's backward gave the tensor back
            mc, fc, cx, cz = fwd(ca)                              # may take the arena's tensor again
            if use_arena:
                assert arena.busy()
            torch.autograd.backward([cx, cz], [torch.sign(cx.detach()), torch.sign(cz.detach())])
            md, fd_, dx, dz = fwd(cb)
            del md, fd_, dx, dz                                   # a graph dropped without a backward frees it too
            if use_arena:
                import gc
                gc.collect()
                assert not arena.busy()
        return [t.grad.clone() for t in (ma, fa, mb, fb, mc, fc)]
    plain, shared = grads(False), grads(True)
    for p, s in zip(plain, shared):
        assert float(p.abs().max()) > 0 and torch.equal(p, s)
    assert torch.equal(plain[0], plain[4])                        # the third pass repeats the first
